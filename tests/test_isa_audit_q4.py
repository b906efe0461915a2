"""ISA audit of the 4-bit GPTQ instantiations of the streaming decode kernel (gemv_stream_kernel, WT = 3) -- runs WITHOUT a GPU: hipcc
cross-compiles tests/native/q4_isa_probe.hip, which holds each audited 4-bit instantiation next to the 16-bit instantiation (WT = 1) of the same
form, and the properties the 4-bit mode must have are asserted on the text:
  * no scratch (a spill's traffic shares vmcnt with the weight stream);
  * the fine-grid forms still fit two blocks per CU (<= 256 VGPRs; their LDS is sized on the host, <= 80 KiB);
  * the same v_mfma_f32_16x16x32 count as the 16-bit form (the dequantisation adds VALU work, never a matrix instruction);
  * no `s_waitcnt vmcnt(0)` inside a stage that the 16-bit form does not have: the stage bodies are the instruction runs between consecutive
    MFMAs that do not cross a tile end (the tile end holds the s_barrier and the epilogue, where both forms wait for their late loads);
  * ONE weight load instruction per stage (the 16-bit form has four), and the dequantisation is the packed fp16 subtract / multiply.
The audited forms are those of up to 8 tenants.  The 12- and 16-tenant forms (plain and SwiGLU launches only) fill all 512 VGPRs and spill in
EVERY weight form, the 16-bit one included (about 1 KB of scratch per lane at 16 tenants, about the same amount in all three): that is
inherited, not audited here, and "no scratch" is not claimed for them."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# (DT, NM, NS of the 16-bit form, NS of the 4-bit form, XL, EPI, FG) of the probe's pairs, each at its shipped prefetch depth.  The mangled
# name spells every template argument as Li<value>E / Lb1E.
FORMS = [(0, 6, 4, 4, 0, 0, 0), (1, 1, 3, 6, 0, 0, 0), (1, 6, 2, 2, 1, 1, 0), (0, 6, 2, 2, 2, 0, 0), (1, 8, 2, 2, 3, 1, 0), (0, 6, 2, 2, 3, 0, 1),
         (1, 6, 2, 2, 2, 1, 1), (0, 1, 2, 8, 3, 1, 0), (1, 2, 2, 8, 3, 0, 1), (1, 1, 2, 8, 1, 0, 0)]


def _key(dt, nm, ns, xl, epi, wt, fg):
    return "gemv_stream_kernelILi%dELi%dELb1ELi%dELi4ELi1ELi2ELi1ELi%dELi%dELi%dELi%dEE" % (dt, nm, ns, xl, epi, wt, fg)


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    import isa_gaps
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("isa") / "q4.s"
    src = os.path.join(ROOT, "tests", "native", "q4_isa_probe.hip")
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


@pytest.mark.parametrize("form", FORMS, ids=lambda f: "DT%d-NM%d-NS%d-NSQ%d-XL%d-EPI%d-FG%d" % f)
def test_q4_instantiation_against_its_16_bit_twin(kernels, form):
    dt, nm, ns, nsq, xl, epi, fg = form
    assert nsq % ns == 0
    dep = nsq // ns
    w16, w4 = _one(kernels, _key(dt, nm, ns, xl, epi, 1, fg)), _one(kernels, _key(dt, nm, nsq, xl, epi, 3, fg))
    for body in (w16, w4):
        assert _meta(body, "amdhsa_private_segment_fixed_size") == 0
        assert not any("scratch_" in l for l in body)
    if fg:
        assert _meta(w4, "amdhsa_next_free_vgpr") <= 256, "two blocks per CU"
    else:
        assert _meta(w4, "amdhsa_next_free_vgpr") <= 512
    i16, s16 = _stage_bodies(w16)
    i4, s4 = _stage_bodies(w4)
    # NS stages x 4 steps x (base + NM masks) MFMAs per unrolled round: the dequantisation adds VALU work, never a matrix instruction
    assert len(i4) == dep * len(i16) and len(i16) % (ns * 4 * (nm + 1)) == 0, (len(i4), len(i16))
    drains = lambda runs: sum(1 for r in runs for l in r if "vmcnt(0)" in l)
    assert drains(s4) <= dep * drains(s16), (drains(s4), drains(s16))      # (per stage: no more than the 16-bit form)

    def pre_barrier_drains(body, idx):
        n = 0
        for a, b in zip(idx, idx[1:]):
            run = body[a + 1:b]
            bar = next((k for k, l in enumerate(run) if "s_barrier" in l), None)
            if bar is not None:
                n += sum(1 for l in run[:bar] if "vmcnt(0)" in l)
        return n
    assert pre_barrier_drains(w4, i4) <= dep * pre_barrier_drains(w16, i16), (pre_barrier_drains(w4, i4), pre_barrier_drains(w16, i16))
    head = lambda body, idx: sum(1 for l in body[:idx[0]] if "vmcnt(0)" in l)
    assert head(w4, i4) <= head(w16, i16), "a full drain in front of the first stage"
    # one weight load per stage: the weight stream is the only one with the nt policy (probe: AUX = 2).  The prologue issues NS stages, the
    # unrolled rounds one per stage they consume (4 (NM + 1) MFMAs each); the 16-bit twin issues at least four per stage
    nt = lambda b: sum(1 for l in b if re.search(r"buffer_load_dwordx4.*\bnt\b", l))
    assert nt(w4[:i4[0]]) == nsq and nt(w4[i4[0]:]) == len(i4) // (4 * (nm + 1)), (nt(w4[:i4[0]]), nt(w4[i4[0]:]), len(i4))
    assert nt(w16[:i16[0]]) >= 4 * ns, "the twin's prologue: four per stage (hipcc may duplicate some under its branches)"
    # ... and between two MFMAs of the main loop at most one of them is issued
    assert max(sum(1 for l in r if re.search(r"buffer_load_dwordx4.*\bnt\b", l)) for r in s4) <= 1
    # the dequantisation: packed fp16 subtract and multiply in the 4-bit form only, one each per element pair (16 pairs per lane and stage);
    # bf16 adds the packing convert
    # (counted over the whole kernel: the first step's fragment of a round is built in front of the round's first MFMA)
    cnt = lambda b, i, pat: sum(1 for l in b if pat in l)
    assert cnt(w16, i16, "v_pk_mul_f16") == 0 and cnt(w4, i4, "v_pk_mul_f16") >= 16 * nsq
    assert cnt(w4, i4, "v_pk_add_f16") >= 16 * nsq
    if dt == 1:
        assert cnt(w4, i4, "v_cvt_pk_bf16_f32") >= 16 * nsq


def test_fine_grid_lds_budget_is_unchanged():
    """the 4-bit mode adds no LDS: the fine-grid kernels' own area + the rows are what the host sizes, <= 80 KiB (two blocks per CU)"""
    txt = open(os.path.join(ROOT, "bitdelta_amd", "csrc", "bd_gemv_stream.h")).read()
    assert re.search(r"STREAM_FG_LDS_MAX = 80 \* 1024", txt)
    assert "WT == 3" in txt and "WT <= 3" in txt
    kernel = txt[txt.index("gemv_stream_kernel(const StreamParams sp)"):]
    assert len(re.findall(r"__shared__", kernel)) == 1, "the 4-bit mode declares no LDS of its own: one dynamic array, sized on the host"
