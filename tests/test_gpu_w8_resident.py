"""TenantDecoder(base_int8=True, dense_base=False): the int8 bytes are the one resident copy of every delta Linear's base and every launch with
more than one row per tenant runs bd_binary_linear_w8 on them.  Reference: tenant t's dense fp32 model from CB * SCB / 127 + alpha * S
(test_gpu_w8_decode.unrounded_twin), 3e-3 as there; session tokens pass test_gpu_session_extend._truth."""
import pytest
import torch

pytestmark = pytest.mark.gpu

CFG, T, SEED, MORE = (1024, 2048, 1, 8, 2, 512), 3, 5, [11, 402, 77, 3, 250]
PROMPTS = [[(7 * t + 3 * i) % 500 + 1 for i in range(n)] for t, n in enumerate((9, 33, 20))]


def _session_turns(dec):
    sess = dec.session()
    for t, p in enumerate(PROMPTS):
        sess.submit(t, p, max_new_tokens=8)
    sess.run()
    turns = [sess.result(1)[0]]
    for more in (MORE, []):                     # tenant 1 extended by 5 tokens, then by none (a one-row chunk)
        sess.extend(1, more, max_new_tokens=4)
        sess.run()
        turns.append(sess.result(1)[0])
    return turns


def _check_turns(bd, twin, turns):
    from test_gpu_session_extend import _truth
    hist = list(PROMPTS[1])
    for more, turn in zip(([], MORE, []), turns):
        hist += more
        _truth(bd, twin, 1, 64 - len(PROMPTS[1]), hist, turn)
        hist += turn.tolist()


def test_resident_int8_decoder_keeps_one_copy_and_matches_the_dense_model():
    import bitdelta_amd as bd
    from test_gpu_serving import _dense_reference_logits, relerr
    from test_gpu_w8_decode import unrounded_twin
    from bitdelta_amd.serving_loop import TenantDecoder
    dec = TenantDecoder.synthetic(CFG, T, "cuda", dtype=torch.float16, seed=SEED, max_len=256, base_int8=True, dense_base=False)
    for name in ("qkv", "o", "gate_up", "down"):
        fl = getattr(dec.layers[0], name)
        assert fl.weight is None and fl.weight_tiled.dtype == torch.int8 and "weight" not in fl.state_dict()
        assert fl.linear_bytes() == fl.N * fl.K + fl.mask.numel() * 4
    twin = unrounded_twin(dec)
    ids, am = dec.prepare(PROMPTS)
    lg = dec.prefill(ids, am, dec.new_cache()).float()
    for t in range(T):
        e = relerr(lg[t], _dense_reference_logits(bd, twin, t, ids[t], am[t]))
        assert e <= 3e-3, (t, e)
    _check_turns(bd, twin, _session_turns(dec))


def test_default_decoder_hands_the_16_bit_weight_to_every_prefill_launch(monkeypatch):
    import bitdelta_amd as bd
    from bitdelta_amd import serving_loop as sl
    from test_gpu_w8_decode import unrounded_twin
    dec = sl.TenantDecoder.synthetic(CFG, T, "cuda", dtype=torch.float16, seed=SEED, max_len=256, base_int8=True)
    dense = {getattr(dec.layers[0], n).weight.data_ptr() for n in ("qkv", "o", "gate_up", "down")}
    seen, orig = [], sl.binary_linear
    monkeypatch.setattr(sl, "binary_linear", lambda x, w, *a, **kw: (seen.append((w.dtype, w.data_ptr())), orig(x, w, *a, **kw))[1])
    turns = _session_turns(dec)
    assert seen and all(dt == torch.float16 and ptr in dense for dt, ptr in seen)
    _check_turns(bd, unrounded_twin(dec), turns)
