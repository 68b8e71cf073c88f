"""``ddsp_svc_amd._modules.packed_table`` and ``ddsp_svc_amd._patching`` on the CPU: no library, no emulator.  The ``pack`` function
here writes a marker into the host table it returns and counts its calls."""
import gc
import types
import weakref

import pytest
import torch

from ddsp_svc_amd import _modules as M
from ddsp_svc_amd import _patching as P

CPU = torch.device("cpu")


class Packer:
    """a caller's ``pack``: the host table of ``n`` floats, a marker written into it; counts its calls"""

    def __init__(self, n=4, marker=7.0):
        self.calls, self.n, self.marker = 0, n, marker

    def __call__(self, dims, tensors):
        self.calls += 1
        return self.marker + torch.arange(self.n, dtype=torch.float32)


@pytest.fixture(autouse=True)
def empty_cache():
    M.clear_packed()
    yield
    M.clear_packed()


def _tensors(n=2, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.rand(3, generator=g) for _ in range(n)]


def test_table_is_float32_of_nbytes_and_holds_what_pack_wrote():
    pack = Packer(6, 5.0)
    table = M.packed_table("resblock", (16, 3), _tensors(), CPU, pack)
    assert table.dtype == torch.float32 and table.shape == (6,) and table.device == CPU
    assert table.tolist() == [5.0, 6.0, 7.0, 8.0, 9.0, 10.0] and pack.calls == 1


def test_two_kinds_are_two_tables():
    ts, pack = _tensors(), Packer()
    a = M.packed_table("resblock", (16, 3), ts, CPU, pack)
    b = M.packed_table("seam", (16, 3), ts, CPU, pack)
    assert a is not b and pack.calls == 2 and len(M._PACKED) == 2
    c = M.packed_table("seam", (16, 4), ts, CPU, pack)                       # and other dims another
    assert c is not b and pack.calls == 3


def test_repeat_is_the_same_object_without_a_pack():
    ts, pack = _tensors(), Packer()
    a = M.packed_table("conformer", (256, True), ts, CPU, pack)
    assert M.packed_table("conformer", (256, True), list(ts), CPU, pack) is a and pack.calls == 1


def test_in_place_write_packs_again():
    ts, pack = _tensors(), Packer()
    a = M.packed_table("seam", (16, 2, 2), ts, CPU, pack)
    ts[1].add_(0)
    b = M.packed_table("seam", (16, 2, 2), ts, CPU, pack)
    assert b is not a and pack.calls == 2 and len(M._PACKED) == 1
    assert M.packed_table("seam", (16, 2, 2), ts, CPU, pack) is b and pack.calls == 2


def test_bound_of_256_entries_first_in_first_out():
    sets, pack = [[torch.zeros(1)] for _ in range(257)], Packer()
    for ts in sets:
        M.packed_table("resblock", (16, 3), ts, CPU, pack)
        assert len(M._PACKED) <= 256
    assert pack.calls == 257 and len(M._PACKED) == 256
    M.packed_table("resblock", (16, 3), sets[256], CPU, pack)                 # the newest is still there
    assert pack.calls == 257
    M.packed_table("resblock", (16, 3), sets[0], CPU, pack)                   # the oldest went, and takes the next oldest's place
    assert pack.calls == 258 and len(M._PACKED) == 256
    M.packed_table("resblock", (16, 3), sets[1], CPU, pack)
    assert pack.calls == 259


def test_entry_keeps_its_tensors_alive():
    ts, pack = _tensors(), Packer()
    ref = weakref.ref(ts[0])
    M.packed_table("resblock", (16, 3), ts, CPU, pack)
    del ts
    gc.collect()
    assert ref() is not None                                                    # so its data_ptr cannot become another tensor's
    M.clear_packed()
    gc.collect()
    assert ref() is None


def test_clear_packed_empties_the_cache():
    ts, pack = _tensors(), Packer()
    M.packed_table("resblock", (16, 3), ts, CPU, pack)
    assert len(M._PACKED) == 1
    M.clear_packed()
    assert len(M._PACKED) == 0
    M.packed_table("resblock", (16, 3), ts, CPU, pack)
    assert pack.calls == 2


def test_failed_pack_raises_and_caches_nothing():
    def refuses(dims, tensors):
        raise ValueError("outside the kernel's range")
    with pytest.raises(ValueError):
        M.packed_table("resblock", (16, 3), _tensors(), CPU, refuses)
    assert len(M._PACKED) == 0


# ---- park / unpark ------------------------------------------------------------------------------------------------------------

def _owner():
    class Net:
        def forward(self):
            return "original"
    return Net, Net.forward


def test_second_park_after_the_swap_returns_the_first_original():
    Net, orig = _owner()
    assert P.park(Net, "forward") is orig and Net._reference_forward is orig
    Net.forward = lambda self: "mine"
    assert P.park(Net, "forward") is orig and Net._reference_forward is orig
    assert Net().forward() == "mine"


def test_unpark_restores_and_removes():
    Net, orig = _owner()
    P.park(Net, "forward")
    Net.forward = lambda self: "mine"
    P.unpark(Net, "forward")
    assert Net.forward is orig and "_reference_forward" not in vars(Net) and Net().forward() == "original"


def test_unpark_of_a_name_never_parked_changes_nothing():
    Net, orig = _owner()
    before = dict(vars(Net))
    P.unpark(Net, "forward")
    P.unpark(Net, "absent")
    assert dict(vars(Net)) == before and Net.forward is orig


def test_subclass_of_a_parked_class_parks_its_own():
    Net, orig = _owner()
    P.park(Net, "forward")
    Net.forward = lambda self: "mine"

    class Sub(Net):
        def forward(self):
            return "sub"
    sub = Sub.forward
    assert Sub._reference_forward is orig                                       # inherited: not the subclass's own original
    assert P.park(Sub, "forward") is sub and vars(Sub)["_reference_forward"] is sub and Net._reference_forward is orig
    Sub.forward = lambda self: "mine too"
    P.unpark(Sub, "forward")
    assert Sub.forward is sub and "_reference_forward" not in vars(Sub) and Net._reference_forward is orig


def test_park_on_a_module():
    mod = types.ModuleType("somewhere")
    mod.f = orig = lambda: 1
    assert P.park(mod, "f") is orig and mod._reference_f is orig
    mod.f = lambda: 2
    P.unpark(mod, "f")
    assert mod.f is orig and not hasattr(mod, "_reference_f")


# ---- undo_rebound ---------------------------------------------------------------------------------------------------------------

def test_undo_rebound_leaves_what_somebody_else_changed():
    old, new, theirs = object(), object(), object()
    a, b, c = (types.SimpleNamespace(f=new) for _ in range(3))
    b.f = theirs                                                                # changed after the rebind
    del c.f                                                                     # or removed
    changed = [(a, "f", old, new), (b, "f", old, new), (c, "f", old, new)]
    P.undo_rebound(changed)
    assert a.f is old and b.f is theirs and not hasattr(c, "f") and changed == []


def test_rebind_everywhere_finds_by_identity_and_skips_parked_names(monkeypatch):
    import sys
    orig, new = object(), object()
    m1, m2, m3 = (types.ModuleType("rebind_case_%d" % i) for i in range(3))
    m1.thing, m1._reference_thing, m2.alias, m3.thing = orig, orig, orig, orig
    for m in (m1, m2, m3):
        monkeypatch.setitem(sys.modules, m.__name__, m)
    changed = P.rebind_everywhere({orig: new}, skip=[m3])
    assert sorted((m.__name__, n) for m, n, _o, _n in changed) == [("rebind_case_0", "thing"), ("rebind_case_1", "alias")]
    assert m1.thing is new and m1._reference_thing is orig and m2.alias is new and m3.thing is orig
    P.undo_rebound(changed)
    assert m1.thing is orig and m2.alias is orig
