"""ISA audit of the int8-base instantiations of the streaming decode kernel (gemv_stream_kernel, WT = 2) -- runs WITHOUT a GPU: hipcc
cross-compiles tests/native/w8_isa_probe.hip, which holds each audited int8 instantiation next to the 16-bit instantiation (WT = 1) of the same
form, and the properties the int8 mode must not lose are asserted on the text:
  * no scratch (a spill's traffic shares vmcnt with the weight stream);
  * the fine-grid forms still fit two blocks per CU (<= 256 VGPRs; their LDS is sized on the host, <= 80 KiB);
  * the same v_mfma_f32_16x16x32 count as the 16-bit form (the widening adds VALU work, never a matrix instruction), every weight widened by
    one byte-select convert;
  * no `s_waitcnt vmcnt(0)` inside a stage that the 16-bit form does not have: the stage bodies are the instruction runs between consecutive
    MFMAs that do not cross a tile end (the tile end holds the s_barrier and the epilogue, where both forms wait for their late loads)."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# (DT, NM, NS of the 16-bit form, XL, EPI, FG) of the probe's pairs, each at its shipped prefetch depth: with one or two tenants the int8 twin runs 2 NS
# stages (half the bytes per stage), from four tenants on the same NS.  The mangled name spells every template argument as Li<value>E / Lb1E.
FORMS = [(0, 6, 4, 0, 0, 0), (1, 1, 3, 0, 0, 0), (1, 6, 2, 1, 1, 0), (0, 6, 2, 2, 0, 0), (1, 8, 2, 3, 1, 0), (0, 6, 2, 3, 0, 1), (1, 6, 2, 2, 1, 1), (0, 1, 2, 3, 1, 0), (1, 2, 2, 3, 0, 1)]


def _key(dt, nm, ns, xl, epi, wt, fg):
    return "gemv_stream_kernelILi%dELi%dELb1ELi%dELi4ELi1ELi2ELi1ELi%dELi%dELi%dELi%dEE" % (dt, nm, ns, xl, epi, wt, fg)


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    import isa_gaps
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("isa") / "w8.s"
    src = os.path.join(ROOT, "tests", "native", "w8_isa_probe.hip")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-pass-failed", "--cuda-device-only", "-S", "-o", str(out), src])
    ks = {name: body for name, body in isa_gaps.kernels(str(out)) if "gemv_stream_kernel" in name}
    assert len(ks) == 2 * len(FORMS)
    return ks


def _one(ks, key):
    hits = [b for n, b in ks.items() if key in n]
    assert len(hits) == 1, key
    return hits[0]


def _meta(body, key):
    m = re.search(r"\." + key + r"\s+(\d+)", "\n".join(body))
    assert m, key
    return int(m.group(1))


def _stage_bodies(body):
    """instruction runs between consecutive MFMAs that hold no s_barrier (a run with one is a tile end: reduction + epilogue)"""
    idx = [i for i, l in enumerate(body) if "v_mfma_f32_16x16x32" in l]
    return idx, [body[a + 1:b] for a, b in zip(idx, idx[1:]) if not any("s_barrier" in l for l in body[a + 1:b])]


@pytest.mark.parametrize("form", FORMS, ids=lambda f: "DT%d-NM%d-NS%d-XL%d-EPI%d-FG%d" % f)
def test_int8_instantiation_against_its_16_bit_twin(kernels, form):
    dt, nm, ns, xl, epi, fg = form
    dep = 2 if nm <= 2 else 1
    w16, w8 = _one(kernels, _key(dt, nm, ns, xl, epi, 1, fg)), _one(kernels, _key(dt, nm, dep * ns, xl, epi, 2, fg))
    for body in (w16, w8):
        assert _meta(body, "amdhsa_private_segment_fixed_size") == 0
        assert not any("scratch_" in l for l in body)
    if fg:
        assert _meta(w8, "amdhsa_next_free_vgpr") <= 256, "two blocks per CU"
    else:
        assert _meta(w8, "amdhsa_next_free_vgpr") <= 512
    i16, s16 = _stage_bodies(w16)
    i8, s8 = _stage_bodies(w8)
    # NS stages x 4 steps x (base + NM masks) MFMAs per unrolled round: the widening adds VALU work, never a matrix instruction
    assert len(i8) == dep * len(i16) and len(i16) % (ns * 4 * (nm + 1)) == 0, (len(i8), len(i16))
    drains = lambda runs: sum(1 for r in runs for l in r if "vmcnt(0)" in l)
    assert drains(s8) <= dep * drains(s16), (drains(s8), drains(s16))      # (per stage: no more than the 16-bit form)
    # ... and none in front of a tile end's barrier either: every wave passes there, a drain would stall the whole block once per tile (the
    # first version of the int8 stage loads had one: hipcc had wrapped their offsets in divergent branches)
    def pre_barrier_drains(body, idx):
        n = 0
        for a, b in zip(idx, idx[1:]):
            run = body[a + 1:b]
            bar = next((k for k, l in enumerate(run) if "s_barrier" in l), None)
            if bar is not None:
                n += sum(1 for l in run[:bar] if "vmcnt(0)" in l)
        return n
    assert pre_barrier_drains(w8, i8) <= dep * pre_barrier_drains(w16, i16), (pre_barrier_drains(w8, i8), pre_barrier_drains(w16, i16))
    head = lambda body, idx: sum(1 for l in body[:idx[0]] if "vmcnt(0)" in l)
    assert head(w8, i8) <= head(w16, i16), "a full drain in front of the first stage"
    # the widening: sign-extending byte converts in the int8 form only, 32 weights per lane and stage
    cvt = lambda b: sum(1 for l in b[i8[0] if b is w8 else i16[0]:] if "v_cvt_f32_i32" in l)
    assert cvt(w16) == 0 and cvt(w8) >= 24 * dep * ns, (cvt(w16), cvt(w8))


def test_fine_grid_lds_budget_is_unchanged():
    """the int8 mode adds no LDS: the fine-grid kernels' own area + the rows are what the host sizes, <= 80 KiB (two blocks per CU)"""
    txt = open(os.path.join(ROOT, "bitdelta_amd", "csrc", "bd_gemv_stream.h")).read()
    assert re.search(r"STREAM_FG_LDS_MAX = 80 \* 1024", txt)
    assert "WT == 2" in txt and "dyn_lds" in txt
    kernel = txt[txt.index("gemv_stream_kernel(const StreamParams sp)"):]
    assert len(re.findall(r"__shared__", kernel)) == 1, "the int8 mode declares no LDS of its own: one dynamic array, sized on the host"
    api = open(os.path.join(ROOT, "bitdelta_amd", "csrc", "bd_api.hip")).read()
    assert "FG == 1 ? STREAM_FG_LDS_MAX : STREAM_LDS_MAX" in api
