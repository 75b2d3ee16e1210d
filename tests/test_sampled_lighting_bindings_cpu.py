"""The two sampled-lighting wrappers of rt64.py (sample_lighting, trace_sampled_lighting) against the stub library of tests/test_query_bindings_cpu.py: which
entry point each calls, with which arguments in which order, what it allocates, what it converts, how keys and the two overrides travel (NULL when not given),
what it refuses and with which words.  No GPU and no librt64.so.
"""
import ctypes

import numpy as np
import pytest

from sm64rt_legacy_renderer_amd import rt64
from test_query_bindings_cpu import LODS, N, TWO_ARRAYS, ONE_ARRAY, VIEW, StubLibrary, _lods, _outputs, _rays

KEYS = "keys: an (N, 4) uint32 array"


class KeyStub(StubLibrary):
    """The stub, which also copies the keys and the RT64_LIGHT_SAMPLING a wrapper hands over while the call runs."""

    def __getattr__(self, name):
        inner = StubLibrary.__getattr__(self, name)

        def entry(*args):
            for role, a in zip(self.roles, args[1:]):
                if role == "keys" and a is not None:
                    self.seen[role] = np.ctypeslib.as_array((ctypes.c_uint32 * (N * 4)).from_address(a)).reshape(N, 4).copy()
                if role == "sampling" and a is not None:
                    s = rt64.LIGHT_SAMPLING.from_address(a)
                    self.seen[role] = (s.maxLights, s.diSamples, s.flags, s.reserved)
            return inner(*args)
        return entry


def _keys(n=N):
    return (np.arange(n * 4, dtype=np.uint32).reshape(n, 4) * 77 + 3)


# name, call(lib, rays, hits, lods, keys, overrides, flags), entry point, argument roles in order, output widths
WRAPPERS = [
    ("sample_lighting", lambda lib, r, h, l, k, o, f: rt64.sample_lighting(lib, VIEW, r, h, l, k, *o), "SampleViewRayLights",
     ("rays", "hits", "lods", "keys", "sampling", "out0", "count"), (16,)),
    ("trace_sampled_lighting", lambda lib, r, h, l, k, o, f: rt64.trace_sampled_lighting(lib, VIEW, r, l, k, *o, flags=f), "TraceViewRaySampledLights",
     ("rays", "out0", "lods", "keys", "sampling", "out1", "count", "flags"), (8, 16)),
]
IDS = [w[0] for w in WRAPPERS]


@pytest.mark.parametrize("name,call,entry,roles,widths", WRAPPERS, ids=IDS)
@pytest.mark.parametrize("with_lods", [False, True])
@pytest.mark.parametrize("with_keys", [False, True])
@pytest.mark.parametrize("overrides", [(-1, -1), (16, 0), (-1, 5), (3, -1)])
def test_entry_point_argument_order_and_outputs(name, call, entry, roles, widths, with_lods, with_keys, overrides):
    lib = KeyStub(roles=roles)
    rays, hits, lods, keys = _rays(), _rays() + 100.0, (_lods() if with_lods else None), (_keys() if with_keys else None)
    flags = 0x1
    outs = _outputs(call(lib, rays, hits, lods, keys, overrides, flags), widths)
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
        elif role == "keys":
            assert np.array_equal(lib.seen[role], keys) if with_keys else a is None
        elif role == "sampling":
            assert a is None if overrides == (-1, -1) else lib.seen[role] == (overrides[0], overrides[1], 0, 0)
        elif role.startswith("out"):
            assert a == outs[int(role[3:])].ctypes.data
        elif role == "count":
            assert a == N
        else:
            assert role == "flags" and a == flags
    for o, w in zip(outs, widths):
        assert isinstance(o, np.ndarray) and o.shape == (N, w) and o.dtype == np.float32 and o.flags["C_CONTIGUOUS"]


@pytest.mark.parametrize("name,call,entry,roles,widths", WRAPPERS, ids=IDS)
def test_inputs_are_made_contiguous(name, call, entry, roles, widths):
    lib = KeyStub(roles=roles)
    rays64 = np.asfortranarray(_rays().astype(np.float64))          # float64 and not C-contiguous
    hits_strided = np.repeat(_rays() + 100.0, 2, axis=0)[::2]       # float32, every other row of a larger array
    lods_strided = np.repeat(_lods(), 2).astype(np.float64)[::2]
    keys_strided = np.repeat(_keys().astype(np.int64), 2, axis=0)[::2]          # int64, every other row
    call(lib, rays64, hits_strided, lods_strided, keys_strided, (-1, -1), 0)
    want = {"rays": _rays(), "hits": _rays() + 100.0, "lods": _lods(), "keys": _keys()}
    assert set(lib.seen) == set(roles) & set(want)
    for role, got in lib.seen.items():
        assert got.dtype == (np.uint32 if role == "keys" else np.float32) and np.array_equal(got, want[role]), role


def test_structured_keys_and_the_record_dtype():
    lib = KeyStub(roles=WRAPPERS[0][3])
    keys = np.zeros(N, dtype=rt64.LIGHT_SAMPLE_KEY_DTYPE)
    keys["x"], keys["y"], keys["frame"] = np.arange(N) + 70, np.arange(N) * 3, 63
    out = rt64.sample_lighting(lib, VIEW, _rays(), _rays(), None, keys)
    assert np.array_equal(lib.seen["keys"], np.stack([keys["x"], keys["y"], keys["frame"], keys["reserved"]], axis=1))
    rec = out.view(rt64.RAY_SAMPLED_LIGHTING_DTYPE)
    assert rec.shape == (N, 1) and rec["direct"].shape == (N, 1, 3)


def test_defaults_and_an_empty_batch_go_through():
    lib = StubLibrary()
    empty = np.zeros((0, 8), dtype=np.float32)
    assert rt64.sample_lighting(lib, VIEW, empty, empty).shape == (0, 16)
    hits, records = rt64.trace_sampled_lighting(lib, VIEW, empty)
    assert hits.shape == (0, 8) and records.shape == (0, 16)
    assert lib.calls[0][1][-1] == 0 and lib.calls[0][1][3:6] == (None, None, None)          # count; lods, keys, sampling = NULL
    assert lib.calls[1][1][-2:] == (0, 0) and lib.calls[1][1][3:6] == (None, None, None)    # count, flags


@pytest.mark.parametrize("name,call,entry,roles,widths", WRAPPERS, ids=IDS)
def test_wrong_shapes_raise_value_errors(name, call, entry, roles, widths):
    lib = StubLibrary()
    two = "hits" in roles
    for bad in (np.zeros((N, 7), dtype=np.float32), np.zeros((N * 8,), dtype=np.float32), np.zeros((N, 2, 4), dtype=np.float32)):
        with pytest.raises(ValueError) as e:
            call(lib, bad, bad, None, None, (-1, -1), 0)
        assert str(e.value) == (TWO_ARRAYS if two else ONE_ARRAY)
    for lods in (np.zeros((N, 1), dtype=np.float32), _lods(N + 1), _lods(N - 1)):
        with pytest.raises(ValueError) as e:
            call(lib, _rays(), _rays(), lods, None, (-1, -1), 0)
        assert str(e.value) == LODS
    for keys in (_keys(N + 1), _keys(N - 1), np.zeros((N, 3), dtype=np.uint32), np.zeros((N * 4,), dtype=np.uint32), np.zeros((N, 4), dtype=np.float32)):
        with pytest.raises(ValueError) as e:
            call(lib, _rays(), _rays(), None, keys, (-1, -1), 0)
        assert str(e.value) == KEYS
    assert not lib.calls          # nothing reached the library


@pytest.mark.parametrize("name,call,entry,roles,widths", WRAPPERS, ids=IDS)
def test_a_refusal_raises_with_the_last_error(name, call, entry, roles, widths):
    lib = StubLibrary(status=0)
    with pytest.raises(RuntimeError) as e:
        call(lib, _rays(), _rays(), _lods(), _keys(), (17, 65), 0)          # (out-of-range overrides are the library's to refuse)
    assert str(e.value) == "stub: refused" and len(lib.calls) == 1 and lib.calls[0][0] == entry


def test_the_device_branch_refuses_cpu_tensors():
    """torch tensors select the device branch of sample_lighting; its validation wants CUDA tensors, so CPU tensors reach the checks without a GPU."""
    torch = pytest.importorskip("torch")
    lib = StubLibrary()
    rays, hits = torch.zeros((N, 8)), torch.zeros((N, 8))
    with pytest.raises(ValueError) as e:
        rt64.sample_lighting(lib, VIEW, rays, hits, None, torch.zeros((N, 4), dtype=torch.int32))
    assert str(e.value) == "keys: an (N, 4) int32 or uint32 CUDA tensor"
    with pytest.raises(ValueError) as e:
        rt64.sample_lighting(lib, VIEW, rays, hits)
    assert str(e.value) == "rays, hits: (N, 8) float32 CUDA tensors"
    assert not lib.calls
