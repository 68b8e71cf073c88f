"""``ddsp_svc_amd._modules`` (the packed-table cache, the stacked projections, the routing between a layer's forms, the
predicates) and ``ddsp_svc_amd._patching`` on the CPU: no library, no emulator.  The ``pack`` function here writes a marker into
the host table it returns and counts its calls."""
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


# ---- patch_forwards / unpatch_forwards ----------------------------------------------------------------------------------------

def _reference_module(name="hook_case"):
    """a hand-made module with two classes that have a ``forward`` and one name that is no class of the hook's"""
    mod = types.ModuleType(name)

    class Layer:
        def forward(self, x):
            return ("layer", x)

    class Net:
        def forward(self, x):
            return ("net", x)
    mod.Layer, mod.Net = Layer, Net
    return mod, Layer.forward, Net.forward


def _mine(self, x):
    return ("mine", x)


def _mine_too(self, x):
    return ("mine too", x)


_HOOK = (("Layer", _mine), ("Net", _mine_too), ("Absent", _mine))


def test_patch_forwards_binds_and_unpatch_forwards_undoes():
    mod, layer, net = _reference_module()
    assert P.patch_forwards([mod], _HOOK) == [mod]
    assert mod.Layer.forward is _mine and mod.Net.forward is _mine_too
    assert mod.Layer._reference_forward is layer and mod.Net._reference_forward is net
    assert mod.Layer().forward(3) == ("mine", 3) and not hasattr(mod, "Absent")
    assert P.unpatch_forwards([mod], ["Layer", "Net", "Absent"]) is None
    assert mod.Layer.forward is layer and mod.Net.forward is net
    assert "_reference_forward" not in vars(mod.Layer) and "_reference_forward" not in vars(mod.Net)
    assert mod.Layer().forward(3) == ("layer", 3)


def test_patch_forwards_twice_is_once():
    mod, layer, _ = _reference_module()
    P.patch_forwards([mod], _HOOK)
    other = lambda self, x: ("other", x)
    assert P.patch_forwards([mod], (("Layer", other),)) == [mod]               # not the parked original any more: left alone
    assert mod.Layer.forward is _mine and mod.Layer._reference_forward is layer
    P.unpatch_forwards([mod], ["Layer", "Net"])
    P.unpatch_forwards([mod], ["Layer", "Net"])                                  # and so is the undo
    assert mod.Layer.forward is layer and "_reference_forward" not in vars(mod.Layer)


def test_patch_forwards_on_a_subclass_of_a_patched_class_parks_its_own():
    mod, layer, _ = _reference_module()
    P.patch_forwards([mod], _HOOK)
    sub_mod = types.ModuleType("hook_case_sub")

    class Layer(mod.Layer):
        def forward(self, x):
            return ("sub", x)
    sub_mod.Layer, sub = Layer, Layer.forward
    assert P.patch_forwards([sub_mod], _HOOK) == [sub_mod]
    assert Layer.forward is _mine and vars(Layer)["_reference_forward"] is sub and mod.Layer._reference_forward is layer
    P.unpatch_forwards([sub_mod], ["Layer"])
    assert Layer.forward is sub and "_reference_forward" not in vars(Layer) and mod.Layer.forward is _mine


def test_patch_forwards_takes_names_and_objects_and_skips_what_does_not_import(monkeypatch):
    import sys
    named, layer, _ = _reference_module("hook_case_named")
    given, _, net = _reference_module("hook_case_given")
    monkeypatch.setitem(sys.modules, named.__name__, named)                     # importable by name
    assert "hook_case_that_is_nowhere" not in sys.modules
    done = P.patch_forwards(["hook_case_that_is_nowhere", named.__name__, given], _HOOK)
    assert done == [named, given]                                               # in the order gone through, the missing one left out
    assert named.Layer.forward is _mine and given.Net.forward is _mine_too
    assert P.patch_forwards(["hook_case_that_is_nowhere"], _HOOK) == []
    P.unpatch_forwards(["hook_case_that_is_nowhere", named.__name__, given], ["Layer", "Net"])
    assert named.Layer.forward is layer and given.Net.forward is net
    assert "hook_case_that_is_nowhere" not in sys.modules


# ---- run_reference ------------------------------------------------------------------------------------------------------------

def test_run_reference_prefers_the_parked_forward():
    mod, _, _ = _reference_module()
    P.patch_forwards([mod], _HOOK)
    obj = mod.Layer()
    assert P.run_reference(obj, lambda x, k=0: ("fallback", x), 5) == ("layer", 5)
    assert P.run_reference(obj, None, x=6) == ("layer", 6)                      # called as the method it was, keywords passed on


def test_run_reference_falls_back_when_nothing_is_parked():
    mod, _, _ = _reference_module()
    assert P.run_reference(mod.Layer(), lambda x, k=0: ("fallback", x, k), 5, k=2) == ("fallback", 5, 2)


def test_run_reference_without_either_raises():
    mod, _, _ = _reference_module()
    with pytest.raises(AttributeError):
        P.run_reference(mod.Layer(), None, 5)


# ---- stacked_projection / step_biases -----------------------------------------------------------------------------------------

@pytest.fixture
def no_stacks():
    M._STACKED.clear()
    yield
    M._STACKED.clear()


def _projs(n=3, C=4, seed=0, conv=False):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand((C, C, 1) if conv else (C, C), generator=g), torch.rand(C, generator=g)) for _ in range(n)]


def test_stacked_projection_stacks_and_hits(no_stacks):
    projs = _projs()
    W, b = M.stacked_projection(projs)
    assert torch.equal(W, torch.cat([p[0] for p in projs])) and torch.equal(b, torch.cat([p[1] for p in projs]))
    assert W.shape == (12, 4) and W.is_contiguous() and b.is_contiguous() and not W.requires_grad
    W2, b2 = M.stacked_projection([tuple(p) for p in projs])                    # the same tensors in new containers
    assert W2 is W and b2 is b and len(M._STACKED) == 1


def test_stacked_projection_restacks_after_an_in_place_write(no_stacks):
    projs = _projs()
    W, b = M.stacked_projection(projs)
    projs[1][0].mul_(2.0)
    W2, b2 = M.stacked_projection(projs)
    assert W2 is not W and torch.equal(W2, torch.cat([p[0] for p in projs])) and not torch.equal(W2, W)
    assert len(M._STACKED) == 1 and M.stacked_projection(projs)[0] is W2
    projs[2][1].add_(1.0)                                                       # a bias counts as well
    assert torch.equal(M.stacked_projection(projs)[1], torch.cat([p[1] for p in projs]))


def test_stacked_projection_keeps_its_tensors_alive(no_stacks):
    projs = _projs()
    ref = weakref.ref(projs[0][0])
    M.stacked_projection(projs)
    del projs
    gc.collect()
    assert ref() is not None                                                    # so its data_ptr cannot become another tensor's
    M._STACKED.clear()
    gc.collect()
    assert ref() is None


def test_stacked_projection_bound_of_32_entries_first_in_first_out(no_stacks):
    assert M._STACKED_MAX == 32
    sets = [_projs(1, 2, seed=i) for i in range(33)]
    first = [M.stacked_projection(ps)[0] for ps in sets[:32]]
    assert len(M._STACKED) == 32 and M.stacked_projection(sets[0])[0] is first[0]   # 32 distinct ones are all kept
    M.stacked_projection(sets[32])
    assert len(M._STACKED) == 32                                                # the 33rd dropped the oldest,
    assert M.stacked_projection(sets[31])[0] is first[31]                       # not a newer one
    assert M.stacked_projection(sets[0])[0] is not first[0]


def test_stacked_projection_of_linear_and_conv_weights_is_the_same(no_stacks):
    lin = _projs(3, 4, seed=5)
    conv = [(w.clone().unsqueeze(-1), b.clone()) for w, b in lin]
    assert conv[0][0].shape == (4, 4, 1)
    (Wl, bl), (Wc, bc) = M.stacked_projection(lin), M.stacked_projection(conv)
    assert Wl is not Wc and Wc.shape == (12, 4) and torch.equal(Wl, Wc) and torch.equal(bl, bc)


@pytest.mark.parametrize("B", [0, 1, 3])
def test_step_biases_is_the_addmm_it_replaces(no_stacks, B):
    n, C = 5, 8
    projs, s = _projs(n, C, seed=2, conv=True), torch.rand(B, C, generator=torch.Generator().manual_seed(9))
    W, b = torch.cat([p[0][:, :, 0] for p in projs]), torch.cat([p[1] for p in projs])
    want = torch.addmm(b, s, W.t()).view(B, n, C).transpose(0, 1).contiguous()
    got = M.step_biases(s, projs)
    assert got.shape == (n, B, C) and got.is_contiguous() and torch.equal(got, want)
    for i, (w, bias) in enumerate(projs[:2] if B else []):                      # and each row is that layer's own projection
        assert torch.allclose(got[i], torch.addmm(bias, s, w[:, :, 0].t()), rtol=1e-6, atol=1e-6)


# ---- the routing between the split form, the tiled form and torch -------------------------------------------------------------

def test_split_range_is_whole_tiles_of_16_up_to_4096():
    assert (M.SPLIT_TILE, M.SPLIT_MAX_TILES, M.FORMS) == (16, 4096, ("tiled", "split"))
    assert M.split_in_range(1, 65536) and not M.split_in_range(1, 65537)       # 4096 tiles, and one frame into the 4097th
    assert M.split_in_range(4096, 16) and not M.split_in_range(4096, 17) and M.split_in_range(4096, 1)
    assert M.split_in_range(0, 10 ** 9) and not M.split_in_range(4097, 1)


@pytest.mark.parametrize("below, faster, key, B, n, want", [
    ({}, {}, 512, 1, 100, "tiled"),                       # the key in neither table
    ({384: 8256}, {384: 27584}, 512, 1, 100, "tiled"),    # tables that list another key only
    ({512: 8256}, {512: 27584}, 512, 1, 100, "split"),    # below SPLIT_BELOW and in range
    ({512: 8256}, {512: 27584}, 512, 48, 171, "split"),   # 8 208 frames, 528 tiles
    ({512: 8256}, {512: 27584}, 512, 48, 172, None),      # exactly at the split bound: the side above it, here torch's
    ({512: 8256}, {}, 512, 48, 172, "tiled"),             # ... and here the tiled form's
    ({512: 8256}, {512: 27584}, 512, 32, 862, "tiled"),   # exactly at the torch bound: the side above it
    ({512: 8256}, {512: 27584}, 512, 1, 27583, None),     # one frame below it
    ({512: 10 ** 6}, {512: 27584}, 512, 4097, 1, None),   # below SPLIT_BELOW, 4097 tiles: out of range, falls through to torch
    ({512: 10 ** 6}, {}, 512, 4097, 1, "tiled"),          # ... and to the tiled form
    ({512: 10 ** 6}, {512: 27584}, 512, 4096, 17, "tiled"),   # 8192 tiles of 69 632 frames: past both
    ({512: 10 ** 6}, {512: 27584}, 512, 4096, 16, "split"),   # 4096 tiles exactly are in range
    ({}, {512: None}, 512, 1, 1, None),                   # a torch bound of None: torch at every size
    ({}, {512: None}, 512, 64, 10 ** 6, None),
    ({512: 8256}, {512: None}, 512, 1, 100, "split"),     # the split table is asked first
    ({512: 8256}, {512: None}, 512, 48, 172, None),
])
def test_choose_form_cases(below, faster, key, B, n, want):
    assert M.choose_form(below, faster, key, B, n) == want


def test_the_hooks_route_by_their_own_tables_as_they_are_at_the_call(monkeypatch):
    from ddsp_svc_amd import naive_v2 as NV
    from ddsp_svc_amd import wavenet as WN
    for mod, key in ((WN, 384), (NV, 512)):
        assert mod.SPLIT_MAX_TILES == 4096 and mod.FORMS == ("tiled", "split")
        assert mod.split_in_range(1, 65536) and not mod.split_in_range(1, 65537)
        monkeypatch.setattr(mod, "SPLIT_BELOW", {key: 200})
        monkeypatch.setattr(mod, "LAYER_TORCH_FASTER", {key: 300})
        assert [mod.choose_form(key, 1, n) for n in (199, 200, 299, 300)] == ["split", None, None, "tiled"]
        mod.LAYER_TORCH_FASTER.clear()                                          # in place, as the bench tools do
        assert mod.choose_form(key, 1, 200) == "tiled"
        monkeypatch.setattr(mod, "SPLIT_BELOW", {})
        assert mod.choose_form(key, 1, 1) == "tiled"


# ---- pack_host, plain_with_bias, pointwise ------------------------------------------------------------------------------------

def test_pack_host_stages_and_hands_the_entry_pointers_dims_table_and_size(monkeypatch):
    seen = []

    def entry(*args):
        seen.append(args)
        return 0
    monkeypatch.setattr(M._ffi, "check", lambda code: seen.append(("checked", code)))
    a = torch.arange(6, dtype=torch.float64).reshape(2, 3).t()                  # neither float32 nor contiguous
    host = M.pack_host(40, "refused", [a, torch.ones(2)], entry, (7, 9))
    assert host.dtype == torch.float32 and host.shape == (10,) and host.device == CPU
    (pa, pb, d0, d1, ph, nbytes), checked = seen
    assert (d0, d1, ph, nbytes) == (7, 9, host.data_ptr(), 40) and checked == ("checked", 0)
    assert pa != a.data_ptr() and isinstance(pb, int)
    with pytest.raises(ValueError, match="^refused$"):
        M.pack_host(0, "refused", [a], entry, (7, 9))
    assert len(seen) == 2                                                       # a refusal reaches no entry


def test_plain_with_bias_and_pointwise():
    conv = torch.nn.Conv1d(4, 8, 1)
    assert M.plain_with_bias(conv) and M.pointwise(conv, 4, 8)
    assert not M.pointwise(conv, 4, 4) and not M.pointwise(conv, 8, 8)
    assert M.plain_with_bias(torch.nn.Linear(4, 4)) and not M.pointwise(torch.nn.Linear(4, 8), 4, 8)
    assert not M.plain_with_bias(torch.nn.Conv1d(4, 8, 1, bias=False)) and M.plain(torch.nn.Conv1d(4, 8, 1, bias=False))
    assert not M.plain_with_bias(torch.nn.Conv1d(4, 8, 1).double())
    half_bias = torch.nn.Conv1d(4, 8, 1)
    half_bias.bias = torch.nn.Parameter(half_bias.bias.detach().half())
    assert M.plain(half_bias) and not M.plain_with_bias(half_bias)
    hooked = torch.nn.Conv1d(4, 8, 1)
    hooked.register_forward_pre_hook(lambda m, a: None)
    assert not M.plain_with_bias(hooked) and not M.pointwise(hooked, 4, 8)
    for other in (torch.nn.Conv1d(4, 8, 3, padding=1), torch.nn.Conv1d(4, 8, 1, stride=2), torch.nn.Conv1d(4, 8, 1, padding=1),
                  torch.nn.Conv1d(4, 8, 1, groups=2)):
        assert M.plain_with_bias(other) and not M.pointwise(other, 4, 8)
