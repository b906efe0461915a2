"""The fine-tune tag of a slot across COMPLETED loads (TenantDecoder.load_tenant / TenantSession.load_tenant, tag=), on the GPU:
a named tag is stored by either method; A -> B -> A in one slot carries A's tag again and a second slot loaded as A compares equal; a default
load leaves a fresh object; a load refused because the slot is generating leaves the tag alone; nobody else's tag moves; a load that fails
midway leaves a tag that matches nothing."""
import pytest
import torch

from test_gpu_session_extend import _clone_state, _toks

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dec():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from bitdelta_amd import _lib
    from bitdelta_amd.serving_loop import TenantDecoder
    _lib.lib()
    return TenantDecoder.synthetic("tiny128", 4, "cuda", dtype=torch.float16, seed=31, max_len=256)


def _tags(dec):
    return [dec.tenant_tag(t) for t in range(dec.T)]


def _others_untouched(dec, before, *changed):
    return all(dec.tenant_tag(t) is before[t] for t in range(dec.T) if t not in changed)


def test_a_named_tag_is_stored_by_both_load_tenants(dec):
    A = _clone_state(dec.tenant_state(1))
    before = _tags(dec)
    dec.load_tenant(1, _clone_state(A), tag="A")
    assert dec.tenant_tag(1) == "A" and _others_untouched(dec, before, 1)
    sess = dec.session()
    sess.load_tenant(2, _clone_state(A), tag=("family", 7))
    assert dec.tenant_tag(2) == ("family", 7) and dec.tenant_tag(1) == "A" and _others_untouched(dec, before, 1, 2)
    # the slot really holds the fine-tune that was loaded under the tag
    assert torch.equal(dec.embed[2], A["embed"]) and torch.equal(dec.layers[0].norm1[2], A["layers"][0]["norm1"])


def test_a_b_a_in_one_slot_and_the_same_tag_in_another(dec):
    A, B = _clone_state(dec.tenant_state(0)), _clone_state(dec.tenant_state(3))
    sess = dec.session()
    before = _tags(dec)
    sess.load_tenant(1, _clone_state(A), tag="A")
    sess.load_tenant(1, _clone_state(B), tag="B")
    assert dec.tenant_tag(1) == "B" and dec.tenant_tag(1) != "A"
    sess.load_tenant(1, _clone_state(A), tag="A")
    assert dec.tenant_tag(1) == "A"
    dec.load_tenant(2, _clone_state(A), tag="A")
    assert dec.tenant_tag(1) == dec.tenant_tag(2) == "A"
    assert _others_untouched(dec, before, 1, 2) and dec.tenant_tag(0) != "A" and dec.tenant_tag(3) != "A"


@pytest.mark.parametrize("via_session", [False, True], ids=["decoder", "session"])
def test_a_default_load_leaves_a_fresh_tag(dec, via_session):
    A = _clone_state(dec.tenant_state(0))
    loader = dec.session() if via_session else dec
    loader.load_tenant(1, _clone_state(A), tag="A")
    before = _tags(dec)
    loader.load_tenant(1, _clone_state(A))                       # the same weights, untagged: nothing kept under "A" matches any more
    fresh = dec.tenant_tag(1)
    assert fresh != "A" and all(fresh != x for x in before) and _others_untouched(dec, before, 1)
    loader.load_tenant(1, _clone_state(A))
    assert dec.tenant_tag(1) is not fresh and dec.tenant_tag(1) != fresh
    own = dec.tenant_tag(0)                                      # a slot never loaded: its construction tag goes the same way
    loader.load_tenant(0, _clone_state(A))
    assert dec.tenant_tag(0) is not own and dec.tenant_tag(0) != own


def test_a_load_refused_on_a_generating_slot_leaves_the_tag(dec):
    A = _clone_state(dec.tenant_state(0))
    sess = dec.session()
    sess.load_tenant(1, _clone_state(A), tag="A")
    before = _tags(dec)
    sess.submit(1, _toks(9, 5), max_new_tokens=30)
    sess.step(2)
    assert sess.active()[1]
    with pytest.raises(RuntimeError, match="still generating"):
        sess.load_tenant(1, _clone_state(A), tag="B")
    with pytest.raises(RuntimeError, match="still generating"):
        sess.load_tenant(1, _clone_state(A))
    with pytest.raises(TypeError):
        sess.load_tenant(1, _clone_state(A), tag=["unhashable"])
    with pytest.raises(IndexError):
        sess.load_tenant(4, _clone_state(A), tag="B")
    assert dec.tenant_tag(1) == "A" and all(dec.tenant_tag(t) is before[t] for t in range(dec.T))
    sess.run()
    sess.load_tenant(1, _clone_state(A), tag="B")                # retired: the load is taken
    assert dec.tenant_tag(1) == "B"


def test_a_load_that_fails_midway_leaves_a_tag_that_matches_nothing(dec, monkeypatch):
    """the copies of a load are enqueued one after another; when one of them raises, slot t holds partly new weights -- under neither tag"""
    A, B = _clone_state(dec.tenant_state(0)), _clone_state(dec.tenant_state(3))
    dec.load_tenant(1, _clone_state(A), tag="A")
    before = _tags(dec)
    down = dec.layers[-1].down

    def boom(*a, **kw):
        raise RuntimeError("a copy failed")
    monkeypatch.setattr(down, "load_tenant", boom)
    with pytest.raises(RuntimeError, match="a copy failed"):
        dec.load_tenant(1, _clone_state(B), tag="B")
    monkeypatch.undo()
    now = dec.tenant_tag(1)
    assert now != "A" and now != "B" and all(now != x for x in before) and _others_untouched(dec, before, 1)
    dec.load_tenant(1, _clone_state(A), tag="A")                 # (a whole load puts the slot in order again)
    assert dec.tenant_tag(1) == "A"
