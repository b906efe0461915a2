"""The reference's 4-bit GPTQ dequantisation, run for real: bitdelta/misc.py `dequantize_model(model, quantized_model, "4bit")` on a tiny
two-projection module.  Run once where a checkout of the reference is available:

    python tests/golden/make_golden_gptq4.py /path/to/reference

`dequantize_model` imports two class names it uses only as annotations (bitsandbytes' Linear8bitLt, auto_gptq's exllama QuantLinear); both
packages are absent here, so the two modules are stubbed in sys.modules before `import bitdelta.misc`, and a plain nn.Module carrying qweight /
qzeros / scales stands in for the quantised layer.  Writes DATA only:

    gptq4.pt = {case: {"qweight", "qzeros", "scales", "group_size", "weight_fp16", "weight_bf16"}}

random checkpoint tensors and the weights the reference leaves in an fp16 and in a bf16 model.  Cases: `self_attn.q_proj` N = 16, K = 256,
G = 128 (two groups; inside the decode kernel's envelope) and `mlp.down_proj` N = 16, K = 128, G = 32 (four groups; host only).  Both qzeros
hold the nibbles 0 and 15 (z = 1 and z = 16)."""
import os
import sys
import types

import torch
import torch.nn as nn

ref = sys.argv[1]
sys.path.insert(0, ref)
for mod, cls in (("bitsandbytes.nn.modules", "Linear8bitLt"), ("auto_gptq.nn_modules.qlinear.qlinear_exllama", "QuantLinear")):
    parts = mod.split(".")
    for i in range(1, len(parts) + 1):
        sys.modules.setdefault(".".join(parts[:i]), types.ModuleType(".".join(parts[:i])))
    setattr(sys.modules[mod], cls, type(cls, (nn.Module,), {}))
import bitdelta.misc as ref_misc  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
g = torch.Generator().manual_seed(404)


class QLayer(nn.Module):
    def __init__(self, N, K, G):
        super().__init__()
        self.register_buffer("qweight", torch.randint(-2**31, 2**31 - 1, (K // 8, N), generator=g, dtype=torch.int64).to(torch.int32))
        qz = torch.randint(-2**31, 2**31 - 1, (K // G, N // 8), generator=g, dtype=torch.int64)
        qz[0, 0] = (qz[0, 0] & ~0xFF) | 0xF0                     # columns 0 and 1 of group 0: nibble 0 (z = 1) and nibble 15 (z = 16)
        qz[-1, -1] = (qz[-1, -1] | (0xF << 28)) & ~0xF            # ... and the last group's last dword: z = 16 in the sign bits, z = 1 below
        qz = torch.where(qz >= 2**31, qz - 2**32, qz)
        self.register_buffer("qzeros", qz.to(torch.int32))
        self.register_buffer("scales", (torch.rand(K // G, N, generator=g) * 0.01 + 1e-3).half())


def model(layers, dtype):
    m = nn.Module()
    for block, proj, (N, K, G) in layers:
        b = nn.Module()
        setattr(b, proj, nn.Linear(K, N, bias=False).to(dtype))
        setattr(m, block, b)
    return m


SHAPES = [("self_attn", "q_proj", (16, 256, 128)), ("mlp", "down_proj", (16, 128, 32))]
quant = nn.Module()
for block, proj, (N, K, G) in SHAPES:
    b = nn.Module()
    setattr(b, proj, QLayer(N, K, G))
    setattr(quant, block, b)
out = {}
for dtype, key in ((torch.float16, "weight_fp16"), (torch.bfloat16, "weight_bf16")):
    m = model(SHAPES, dtype)
    ref_misc.dequantize_model(m, quant, "4bit")
    for block, proj, (N, K, G) in SHAPES:
        q = getattr(getattr(quant, block), proj)
        c = out.setdefault(f"{block}.{proj}", {"qweight": q.qweight.clone(), "qzeros": q.qzeros.clone(), "scales": q.scales.clone(), "group_size": G})
        w = getattr(getattr(m, block), proj).weight.detach().clone()
        assert w.dtype == dtype and w.shape == (N, K)
        c[key] = w
for c in out.values():
    nib = torch.stack([(c["qzeros"] >> (4 * i)) & 15 for i in range(8)])
    assert bool((nib == 0).any()) and bool((nib == 15).any()) and c["scales"].shape[0] >= 2
path = os.path.join(HERE, "gptq4.pt")
torch.save(out, path)
print("cases:", list(out), "file bytes:", os.path.getsize(path))
