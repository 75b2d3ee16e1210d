"""The three bounce wrappers of rt64.py (bounce_view_ray_hits, trace_view_ray_bounces, trace_view_ray_mirror_chains) against the stub library of
tests/test_query_bindings_cpu.py: which entry point each calls, with which arguments in which order, what it allocates, what it converts, what it refuses and
with which words.  No GPU and no librt64.so.
"""
import numpy as np
import pytest

from sm64rt_legacy_renderer_amd import rt64
from test_query_bindings_cpu import LODS, N, ONE_ARRAY, TWO_ARRAYS, VIEW, StubLibrary, _lods, _outputs, _rays

DEPTH = 3
# name, call(lib, rays, hits, lods, flags), entry point, argument roles in order, output shapes behind N
WRAPPERS = [
    ("bounce_view_ray_hits", lambda lib, r, h, l, f: rt64.bounce_view_ray_hits(lib, VIEW, r, h, l), "BounceViewRayHits",
     ("rays", "hits", "lods", "out0", "out1", "out2", "count"), ((N, 8), (N, 8), (N, 8))),
    ("trace_view_ray_bounces", lambda lib, r, h, l, f: rt64.trace_view_ray_bounces(lib, VIEW, r, l, f), "TraceViewRayBounces",
     ("rays", "out0", "lods", "out1", "out2", "out3", "count", "flags"), ((N, 8), (N, 8), (N, 8), (N, 8))),
    ("trace_view_ray_mirror_chains", lambda lib, r, h, l, f: rt64.trace_view_ray_mirror_chains(lib, VIEW, r, DEPTH, l, f), "TraceViewRayMirrorChains",
     ("rays", "lods", "depth", "out0", "out1", "count", "flags"), ((DEPTH, N, 8), (DEPTH, N, 8))),
]
IDS = [w[0] for w in WRAPPERS]


@pytest.mark.parametrize("name,call,entry,roles,shapes", WRAPPERS, ids=IDS)
@pytest.mark.parametrize("with_lods", [False, True])
def test_entry_point_argument_order_and_outputs(name, call, entry, roles, shapes, with_lods):
    lib = StubLibrary(roles=roles)
    rays, hits, lods = _rays(), _rays() + 100.0, (_lods() if with_lods else None)
    flags = 0x1
    outs = _outputs(call(lib, rays, hits, lods, flags), shapes)
    assert len(lib.calls) == 1
    got, args = lib.calls[0]
    assert got == entry and args[0] == VIEW and len(args) == 1 + len(roles)
    for role, a in zip(roles, args[1:]):
        if role == "rays":
            assert np.array_equal(lib.seen[role], rays)
        elif role == "hits":
            assert np.array_equal(lib.seen[role], hits)
        elif role == "lods":
            assert np.array_equal(lib.seen[role], lods) if with_lods else a is None
        elif role.startswith("out"):
            assert a == outs[int(role[3:])].ctypes.data
        elif role == "count":
            assert a == N
        elif role == "depth":
            assert a == DEPTH
        else:
            assert role == "flags" and a == flags
    for o, shape in zip(outs, shapes):
        assert isinstance(o, np.ndarray) and o.shape == shape and o.dtype == np.float32 and o.flags["C_CONTIGUOUS"]


def test_an_output_switched_off_is_null_and_left_out():
    lib = StubLibrary()
    rays, hits = _rays(), _rays() + 100.0
    only = rt64.bounce_view_ray_hits(lib, VIEW, rays, hits, reflected=False, refracted=False)
    assert isinstance(only, np.ndarray) and only.shape == (N, 8)
    args = lib.calls[0][1]
    assert args[4] == only.ctypes.data and args[5] is None and args[6] is None and args[7] == N
    refl, refr = rt64.bounce_view_ray_hits(lib, VIEW, rays, hits, bounces=False)
    args = lib.calls[1][1]
    assert args[4] is None and args[5] == refl.ctypes.data and args[6] == refr.ctypes.data
    h, refl = rt64.trace_view_ray_bounces(lib, VIEW, rays, bounces=False, refracted=False)
    args = lib.calls[2][1]
    assert lib.calls[2][0] == "TraceViewRayBounces" and args[2] == h.ctypes.data and args[3] is None and args[4] is None and args[5] == refl.ctypes.data and args[6] is None
    assert args[7:] == (N, 0)


@pytest.mark.parametrize("name,call,entry,roles,shapes", WRAPPERS, ids=IDS)
def test_inputs_are_made_contiguous_float32(name, call, entry, roles, shapes):
    lib = StubLibrary(roles=roles)
    rays64 = np.asfortranarray(_rays().astype(np.float64))          # float64 and not C-contiguous
    hits_strided = np.repeat(_rays() + 100.0, 2, axis=0)[::2]       # float32, every other row of a larger array
    lods_strided = np.repeat(_lods(), 2).astype(np.float64)[::2]
    call(lib, rays64, hits_strided, lods_strided, 0)
    want = {"rays": _rays(), "hits": _rays() + 100.0, "lods": _lods()}
    assert set(lib.seen) == set(roles) & set(want)
    for role, got in lib.seen.items():
        assert got.dtype == np.float32 and np.array_equal(got, want[role]), role


def test_default_flags_are_zero_and_an_empty_batch_goes_through():
    lib = StubLibrary()
    empty = np.zeros((0, 8), dtype=np.float32)
    assert [a.shape for a in rt64.bounce_view_ray_hits(lib, VIEW, empty, empty)] == [(0, 8)] * 3
    assert [a.shape for a in rt64.trace_view_ray_bounces(lib, VIEW, empty)] == [(0, 8)] * 4
    hits, bounces = rt64.trace_view_ray_mirror_chains(lib, VIEW, empty, 8)
    assert hits.shape == (8, 0, 8) and bounces.shape == (8, 0, 8)
    assert lib.calls[0][1][-1] == 0 and lib.calls[0][1][3] is None          # count; lods = NULL
    assert lib.calls[1][1][-2:] == (0, 0)                                   # count, flags
    assert lib.calls[2][1][3] == 8 and lib.calls[2][1][-2:] == (0, 0)       # depth; count, flags


@pytest.mark.parametrize("name,call,entry,roles,shapes", WRAPPERS, ids=IDS)
def test_wrong_shapes_raise_value_errors(name, call, entry, roles, shapes):
    lib = StubLibrary()
    two = "hits" in roles
    for bad in (np.zeros((N, 7), dtype=np.float32), np.zeros((N * 8,), dtype=np.float32), np.zeros((N, 2, 4), dtype=np.float32)):
        with pytest.raises(ValueError) as e:
            call(lib, bad, bad, None, 0)
        assert str(e.value) == (TWO_ARRAYS if two else ONE_ARRAY)
    if two:
        for hits in (_rays(N + 1), _rays(N - 1), np.zeros((N, 7), dtype=np.float32)):
            with pytest.raises(ValueError) as e:
                call(lib, _rays(), hits, None, 0)
            assert str(e.value) == TWO_ARRAYS
    for lods in (np.zeros((N, 1), dtype=np.float32), _lods(N + 1), _lods(N - 1)):
        with pytest.raises(ValueError) as e:
            call(lib, _rays(), _rays(), lods, 0)
        assert str(e.value) == LODS
    assert not lib.calls          # nothing reached the library


@pytest.mark.parametrize("name,call,entry,roles,shapes", WRAPPERS, ids=IDS)
def test_a_refusal_raises_with_the_last_error(name, call, entry, roles, shapes):
    lib = StubLibrary(status=0)
    with pytest.raises(RuntimeError) as e:
        call(lib, _rays(), _rays(), _lods(), 0)
    assert str(e.value) == "stub: refused" and len(lib.calls) == 1 and lib.calls[0][0] == entry


def test_the_device_branch_refuses_cpu_tensors():
    """torch tensors select the device branch of bounce_view_ray_hits and of the chain wrapper; its validation wants CUDA tensors, so CPU tensors reach the check
    without a GPU."""
    torch = pytest.importorskip("torch")
    lib = StubLibrary()
    rays, hits, lods = torch.zeros((N, 8)), torch.zeros((N, 8)), torch.zeros((N,))
    with pytest.raises(ValueError) as e:
        rt64.bounce_view_ray_hits(lib, VIEW, rays, hits, lods)
    assert str(e.value) == "rays, hits: (N, 8) float32 CUDA tensors"
    with pytest.raises(ValueError) as e:
        rt64.trace_view_ray_mirror_chains(lib, VIEW, rays, 2, lods)
    assert str(e.value) == "rays: an (N, 8) float32 CUDA tensor"
    assert not lib.calls
