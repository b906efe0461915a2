"""Host side of the int8 base weight of the decode Linear (bitdelta_amd/quant.py, bd_binary_linear_decode_w8) -- no GPU.

The format is the LLM.int8 vector-wise one the reference dequantises in bitdelta/misc.py:72-73: CB int8 [N, K], SCB = per-output-row absmax,
W ~ (CB * SCB[:, None]) / 127.  The reference's `dequantize_8bit` is a closure of a function that imports bitsandbytes, so it cannot be run
here to make a fixture; the checker is that one-line formula restated below."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def reference_dequantize(cb, scb):
    """bitdelta/misc.py:72-73, restated: the int8 codes times the row absmax, over 127, as fp16"""
    return ((cb * scb.unsqueeze(1)) / 127).half()


def _weights(dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn(48, 256, generator=g) * 0.02).to(dtype)
    w[3] = 0                                    # an all-zero row
    w[5, 7] = w[5].abs().max() * 2              # a row whose maximum is positive ...
    w[6, 9] = -w[6].abs().max() * 2             # ... and one whose maximum is negative
    return w


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_quantiser_error_bound_and_edges(dtype):
    from bitdelta_amd.quant import quantize_base_int8
    w = _weights(dtype)
    cb, scb = quantize_base_int8(w)
    assert cb.dtype == torch.int8 and cb.shape == w.shape and scb.dtype == torch.float32 and scb.shape == (w.shape[0],)
    assert torch.equal(scb, w.float().abs().amax(1))
    assert int(cb.abs().max()) <= 127 and int(cb.min()) >= -127
    assert cb[5, 7] == 127 and cb[6, 9] == -127, "the row maximum maps to +-127"
    assert torch.all(cb[3] == 0) and scb[3] == 0, "an all-zero row gives CB = 0, SCB = 0"
    # every row reaches +-127 at its absmax
    assert torch.equal(cb.abs().amax(1)[scb > 0], torch.full((int((scb > 0).sum()),), 127, dtype=torch.int8))
    # half a quantisation step per element, plus one fp32 ulp of the row scale for the fp32 evaluation of the quotient
    w64, deq = w.double(), cb.double() * scb.double()[:, None] / 127
    bound = scb.double()[:, None] / 254 + torch.finfo(torch.float32).eps * scb.double()[:, None]
    assert torch.all((w64 - deq).abs() <= bound), float(((w64 - deq).abs() - bound).max())
    # round half to even on an exact tie: absmax 127 makes the quotient the value itself
    tie = torch.tensor([[127.0, 0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 3.0]])
    assert quantize_base_int8(tie)[0].tolist() == [[127, 0, 2, 2, 0, -2, -2, 3]]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_dequantise_is_the_reference_line(dtype):
    from bitdelta_amd.quant import dequantize_base_int8, quantize_base_int8, weight_scale
    cb, scb = quantize_base_int8(_weights(dtype, seed=1))
    got = dequantize_base_int8(cb, scb, dtype)
    assert got.dtype == dtype and torch.equal(got, reference_dequantize(cb, scb).to(dtype))
    assert torch.equal(weight_scale(scb), scb / 127) and weight_scale(scb).dtype == torch.float32


def _untile(t, N, K):
    """the inverse of the documented order, written element by element from the index map (not from tile_weight_int8's permute)"""
    flat = t.reshape(-1)
    out = torch.empty(N, K, dtype=t.dtype)
    n, k = torch.meshgrid(torch.arange(N), torch.arange(K), indexing="ij")
    tile, c = n // 16, n % 16
    it, r = k // 128, k % 128
    s, g, e = r // 32, (r % 32) // 8, r % 8
    h, j = s // 2, s % 2
    off = (((((tile * (K // 128) + it) * 2 + h) * 16 + c) * 4 + g) * 2 + j) * 8 + e
    out[n, k] = flat[off]
    return out


def test_tile_weight_int8_is_the_documented_permutation():
    from bitdelta_amd.quant import tile_weight_int8
    N, K = 48, 384
    # distinct values: int16 positions viewed through two int8 planes (an int8 matrix cannot hold 18432 distinct values)
    pos = torch.arange(N * K, dtype=torch.int32).reshape(N, K)
    lo, hi = (pos % 251 - 125).to(torch.int8), (pos // 251 - 36).to(torch.int8)
    assert len({(int(a), int(b)) for a, b in zip(lo.reshape(-1)[::7], hi.reshape(-1)[::7])}) == len(lo.reshape(-1)[::7])
    for plane in (lo, hi):
        t = tile_weight_int8(plane)
        assert t.shape == (N, K) and t.dtype == torch.int8 and t.is_contiguous()
        assert torch.equal(_untile(t, N, K), plane)
        assert torch.equal(t.reshape(-1).sort().values, plane.reshape(-1).sort().values)
    # one stage = one contiguous 2-KiB block: tile 1, iteration 2 holds exactly rows 16..31, k 256..383
    t = tile_weight_int8(lo).reshape(N // 16, K // 128, 2048)
    assert torch.equal(t[1, 2].sort().values, lo[16:32, 256:384].reshape(-1).sort().values)
    # ... and a lane's 16 bytes of load h are its k-octets of steps 2 h and 2 h + 1
    c, g, h = 5, 2, 1
    chunk = tile_weight_int8(lo).reshape(N // 16, K // 128, 2, 16, 4, 16)[1, 2, h, c, g]
    want = torch.cat([lo[16 + c, 256 + 32 * (2 * h + j) + 8 * g:][:8] for j in (0, 1)])
    assert torch.equal(chunk, want)
    for bad in (torch.zeros(40, 128, dtype=torch.int8), torch.zeros(32, 192, dtype=torch.int8), torch.zeros(32, 128, dtype=torch.int16)):
        with pytest.raises(AssertionError):
            tile_weight_int8(bad)


def test_header_documents_the_same_index_map():
    """the index map is written down once in the kernel header and once in the C header; both must be the one the test inverts"""
    for path in ("bitdelta_amd/csrc/bd_gemv_stream.h", "include/bitdelta_hip.h"):
        txt = open(os.path.join(ROOT, path)).read()
        assert re.search(r"\[[Nn]/16\]\[[Kk]/128\]\[h\]", txt), path
        assert re.search(r"128 it \+ 32 \(2 h \+ j\) \+ 8 g \+ e", txt), path


def test_abi_symbol_signature_and_refusals():
    from bitdelta_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    L = _lib.lib()
    name = "bd_binary_linear_decode_w8"
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bitdelta_hip.h")).read(), flags=re.S)
    m = re.search(name + r"\s*\(([^;]*)\)\s*;", hdr)
    assert m, "declared in the stable header"
    nargs = len([a for a in m.group(1).split(",") if a.strip()])
    assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs == 29
    assert hasattr(L, name)
    one = ctypes.c_void_p(16)                 # a non-NULL, aligned, never dereferenced pointer: validation comes before device work

    def call(M=1, N=1024, K=2048, w8=one, ws=one, t_pad=2, B=2, dtype=0, out_dtype=0):
        return L.bd_binary_linear_decode_w8(None, w8, ws, None, t_pad, None, None, B, M, N, K, K, K, 1, 1, 1, N, N, dtype, out_dtype, 0,
                                            None, 0, 0.0, 0, None, None, None, None)
    assert call(M=2) != 0 and call(N=1032) != 0 and call(K=2048 + 64) != 0, "M > 1, N % 16, K % 128 are outside the envelope"
    assert call(ws=None) != 0 and call(w8=None) != 0, "NULL scale / weight"
    assert call(t_pad=3) != 0 and call(B=3) != 0 and call(N=256) != 0
    assert call(dtype=2) != 0
    assert call() != 0, "NULL activations / signs / output: refused before any device work"
    assert L.bd_error_string(call(M=2)) == L.bd_error_string(-3) or call(M=2) < 0


def test_python_envelope_refuses_without_touching_a_device():
    """int8 without a scale, a scale without int8, a non-tiled int8 weight: refused by the wrapper itself (CPU tensors never reach the library)"""
    from bitdelta_amd._lib import BitDeltaHipError
    from bitdelta_amd.binary_gemm_kernel import binary_linear_decode
    x = torch.zeros(2, 1, 2048, dtype=torch.float16)
    w8 = torch.zeros(1024, 2048, dtype=torch.int8)
    with pytest.raises((BitDeltaHipError, ValueError, AssertionError)):
        binary_linear_decode(x, w8, torch.zeros(64, 16, 4, 16, 2, dtype=torch.int32), torch.zeros(2, 1), layout="packed", weight_tiled=True,
                             weight_scale=torch.zeros(1024))


def test_linear_bytes_counts_one_byte_per_base_weight():
    import inspect
    from bitdelta_amd import serving_loop as sl
    assert "base_int8" in inspect.signature(sl.FusedDeltaLinear.__init__).parameters
    assert "base_int8" in inspect.signature(sl.TenantDecoder.__init__).parameters
    assert "base_int8" in inspect.signature(sl.TenantDecoder.synthetic).parameters
    assert inspect.signature(sl.FusedDeltaLinear.__init__).parameters["base_int8"].default is False
    assert inspect.signature(sl.TenantDecoder.synthetic).parameters["base_int8"].default is False
