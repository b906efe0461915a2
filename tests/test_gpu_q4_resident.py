"""TenantDecoder(base_gptq4="only"): the tile-major nibbles and the group parameters are the one resident copy of every delta Linear's base,
and every launch with more than one row per tenant runs bd_binary_linear_q4 on them.  Reference: the base_gptq4=True decoder of the same seed,
whose 16-bit `weight` IS the dequantised base (the dense twin of test_gpu_q4_decode), 3e-3 as there; session tokens pass
test_gpu_session_extend._truth."""
import copy

import pytest
import torch
from test_gpu_w8_resident import CFG, PROMPTS, SEED, T, _check_turns, _session_turns

pytestmark = pytest.mark.gpu


def test_resident_q4_decoder_keeps_one_copy_and_matches_the_dense_model():
    import bitdelta_amd as bd
    from test_gpu_serving import _dense_reference_logits, relerr
    from bitdelta_amd.serving_loop import TenantDecoder
    dec = TenantDecoder.synthetic(CFG, T, "cuda", dtype=torch.float16, seed=SEED, max_len=256, base_gptq4="only")
    twin = TenantDecoder.synthetic(CFG, T, "cuda", dtype=torch.float16, seed=SEED, max_len=256, base_gptq4=True)
    for name in ("qkv", "o", "gate_up", "down"):
        fl, ft = getattr(dec.layers[0], name), getattr(twin.layers[0], name)
        assert fl.weight is None and "weight" not in fl.state_dict() and ft.weight is not None
        for buf in ("weight_tiled", "group_params", "mask"):
            assert torch.equal(getattr(fl, buf), getattr(ft, buf)), buf
        assert fl.linear_bytes() == fl.N * fl.K // 2 + (fl.K // fl.group_size) * fl.N * 4 + fl.mask.numel() * 4
    ids, am = dec.prepare(PROMPTS)
    cache = twin.new_cache()
    want = twin.prefill(ids, am, cache)
    lg = dec.prefill(ids, am, dec.new_cache()).float()
    for t in range(T):
        e = relerr(lg[t], _dense_reference_logits(bd, twin, t, ids[t], am[t]))
        assert e <= 3e-3, (t, e)
    # one decode step from the same cache: the same launch in both decoders
    tok, pos = torch.argmax(want, dim=-1), torch.tensor([ids.shape[1]], device="cuda")
    cache["valid"].index_fill_(1, pos, True)
    steps = [d.forward(tok[:, None], pos, c, c["valid"][:, None, None, :]) for d, c in ((twin, cache), (dec, copy.deepcopy(cache)))]
    assert torch.equal(steps[0], steps[1])
    _check_turns(bd, twin, _session_turns(dec))


def test_default_q4_decoder_hands_the_16_bit_weight_to_every_prefill_launch(monkeypatch):
    import bitdelta_amd as bd
    from bitdelta_amd import serving_loop as sl
    dec = sl.TenantDecoder.synthetic(CFG, T, "cuda", dtype=torch.float16, seed=SEED, max_len=256, base_gptq4=True)
    dense = {getattr(dec.layers[0], n).weight.data_ptr() for n in ("qkv", "o", "gate_up", "down")}
    seen, orig = [], sl.binary_linear
    monkeypatch.setattr(sl, "binary_linear", lambda x, w, *a, **kw: (seen.append((w.dtype, w.data_ptr())), orig(x, w, *a, **kw))[1])
    turns = _session_turns(dec)
    assert seen and all(dt == torch.float16 and ptr in dense for dt, ptr in seen)
    _check_turns(bd, dec, turns)
