"""The decode Linear's dispatch, pinned WITHOUT a GPU (csrc/bd_api.hip: stream_plan decides, launch_stream lifts the plan to one instantiation of
stream_shipped's set).  Every form of this Linear produces the same bits by design, so the output tests cannot see a launch that takes the wrong
prefetch depth, cache policy, grid or LDS layout; these two files can:
  * tests/golden/stream_kernel_forms.txt -- the gemv_stream_kernel instantiations the library compiles.  A host-only compile of bd_api.hip lists
    every kernel it would launch as a __device_stub__ symbol; the list must be that file, so a change to the set edits the file on purpose.
  * tests/golden/stream_dispatch.txt -- which instantiation, grid and LDS layout each call takes (tests/golden/make_stream_dispatch_golden.py: the
    real entry points in dry-run mode).  The recorded cases are replayed against the built library and must agree line by line.
The sweep itself must reach every shipped form an entry point can reach, and at least a tenth of it must be refusals."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLDEN)
import make_stream_dispatch_golden as sweep  # noqa: E402

# packed-layout delta-only forms (HASW = 0, PK = 1): compiled, but every entry point that takes the packed layout requires a base weight
UNREACHABLE = {f"gemv_stream_kernel<{dt}, {nm}, false, {3 if nm == 1 else 4}, 4, 1, 0, 1, 0, 0, 0, 0>(bd::StreamParams)"
               for dt in (0, 1) for nm in (1, 2, 4, 6, 8)}


def golden_lines(name):
    with open(os.path.join(GOLDEN, name)) as fh:
        return [l.rstrip("\n") for l in fh if l.strip()]


def test_compiled_stream_kernels_are_the_golden_list(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    nm = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "lib", "llvm", "bin", "llvm-nm")
    nm = nm if os.path.exists(nm) else shutil.which("llvm-nm") or shutil.which("nm")
    assert nm, "no nm / llvm-nm to list the object's symbols (binutils or the ROCm LLVM tools)"
    obj = tmp_path / "bd_api_host.o"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-fPIC", "--cuda-host-only", "-c", "-o", str(obj),
                           os.path.join(ROOT, "bitdelta_amd", "csrc", "bd_api.hip")])
    syms = subprocess.check_output([nm, "-C", str(obj)], text=True).splitlines()
    stubs = [s for s in syms if "__device_stub__" in s and "gemv_stream_kernel<" in s]
    got = sorted("gemv_stream_kernel<" + s.split("gemv_stream_kernel<", 1)[1] for s in stubs)
    want = golden_lines("stream_kernel_forms.txt")
    assert len(want) == 592 and want == sorted(set(want))
    assert got == want, (f"compiled but not listed: {sorted(set(got) - set(want))[:5]}, listed but not compiled: {sorted(set(want) - set(got))[:5]} "
                         "(tests/golden/stream_kernel_forms.txt is edited on purpose, with the dispatch)")
    # ... and the prefill-size tile kernels (TILE_ROWS and its lifter), the generic kernel and the split-k reduce launches: tile_kernel_forms.txt
    tile = ("delta_gemm_kernel<", "delta_gemm_pf_kernel<", "delta_gemm_fx_kernel<", "delta_gemm_w4_kernel<", "delta_gemm_generic_kernel<",
            "splitk_reduce_kernel<", "splitk_reduce_norm_kernel<")
    got = sorted({s.split("__device_stub__", 1)[1] for s in syms if "__device_stub__" in s and s.split("__device_stub__", 1)[1].startswith(tile)})
    want = golden_lines("tile_kernel_forms.txt")
    assert len(want) == 84 and want == sorted(set(want))
    assert got == want, (f"compiled but not listed: {sorted(set(got) - set(want))[:5]}, listed but not compiled: {sorted(set(want) - set(got))[:5]} "
                         "(tests/golden/tile_kernel_forms.txt is edited on purpose, with the dispatch)")


def test_sweep_reaches_every_form_and_refuses_enough():
    lines = golden_lines("stream_dispatch.txt")
    missing, refusals = sweep.coverage(lines)
    assert set(missing) == UNREACHABLE, sorted(set(missing) ^ UNREACHABLE)
    assert refusals >= 0.10, refusals
    assert os.path.getsize(os.path.join(GOLDEN, "stream_dispatch.txt")) <= os.path.getsize(os.path.join(GOLDEN, "golden.pt"))


def test_dispatch_replay_matches_golden():
    import torch
    if torch.cuda.is_available():
        cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
        if cus != sweep.CUS:
            pytest.skip(f"the recording assumes {sweep.CUS} CUs, this device has {cus}")
    L, n = sweep.load()
    want = golden_lines("stream_dispatch.txt")
    got = sweep.sweep(L, n, [sweep.inputs_of(l) for l in want])      # (refuses to issue a case that could leave the streaming kernel)
    assert len(got) == len(want)
    bad = [(g, w) for g, w in zip(got, want) if g != w]
    assert not bad, f"{len(bad)} of {len(want)} cases decide differently; first: got '{bad[0][0]}', recorded '{bad[0][1]}'"
