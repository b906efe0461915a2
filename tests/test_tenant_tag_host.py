"""CPU-only checks of the fine-tune tags a TenantDecoder keeps per slot (serving_loop.py): the optional argument, unique tags at construction,
and every refusal that needs no device leaves the tag alone.  What a COMPLETED load does to the tag needs the device: tests/test_gpu_tenant_tag.py."""
import inspect

import pytest
import torch


def _dec(tenants=3):
    from bitdelta_amd.serving_loop import MODEL_CONFIGS, TenantDecoder
    return TenantDecoder(MODEL_CONFIGS["tiny128"], tenants, "cpu", torch.float16, max_len=96)


def test_both_load_tenants_take_an_optional_tag():
    from bitdelta_amd.serving_loop import TenantDecoder, TenantSession
    for fn in (TenantDecoder.load_tenant, TenantSession.load_tenant):
        p = inspect.signature(fn).parameters
        assert list(p)[:3] == ["self", "t", "state"] and p["tag"].default is None


def test_tags_are_unique_at_construction():
    dec = _dec()
    tags = [dec.tenant_tag(t) for t in range(3)]
    assert len({id(x) for x in tags}) == 3 and all(a != b for i, a in enumerate(tags) for b in tags[i + 1:])
    assert all(dec.tenant_tag(t) is tags[t] for t in range(3))                # reading it does not change it
    other = _dec()
    assert all(other.tenant_tag(t) != dec.tenant_tag(u) for t in range(3) for u in range(3))


def test_a_refused_load_leaves_the_tag_alone():
    from bitdelta_amd._lib import BitDeltaHipError
    dec = _dec()
    tags = [dec.tenant_tag(t) for t in range(3)]
    with pytest.raises(TypeError):                   # an unhashable tag: refused before the state is looked at
        dec.load_tenant(0, None, tag=["a", "list"])
    with pytest.raises(IndexError):                  # a slot the decoder does not have
        dec.load_tenant(3, {"layers": []}, tag="x")
    with pytest.raises(ValueError):                  # a state of another depth
        dec.load_tenant(0, {"layers": [None]}, tag="x")
    dec.embed = dec.final_norm = dec.lm_head = torch.zeros(3, 4, dtype=torch.float16)
    row = torch.zeros(4, dtype=torch.float16)
    with pytest.raises(BitDeltaHipError):            # a state in order, and no device to load it on
        dec.load_tenant(0, {"layers": [], "embed": row, "final_norm": row, "lm_head": row}, tag="x")
    assert all(dec.tenant_tag(t) is tags[t] for t in range(3))
