"""The four indirect-light wrappers of rt64.py (gi_rays, shade_gi_rays, sample_indirect, trace_indirect) against the stub library of tests/test_query_bindings_cpu.py:
which entry point each calls, with which arguments in which order, what it allocates, what it converts, how keys, incoming light and the three overrides travel (NULL
when not given), what it refuses and with which words.  No GPU and no librt64.so.
"""
import ctypes

import numpy as np
import pytest

from sm64rt_legacy_renderer_amd import rt64
from test_query_bindings_cpu import LODS, N, ONE_ARRAY, VIEW, StubLibrary, _at, _lods, _rays

KEYS = "keys: an (N, 4) uint32 array"
LAYERS = 3


class GiStub(StubLibrary):
    """The stub, which also copies the keys, the layer records, the incoming light and the RT64_GI_SAMPLING a wrapper hands over while the call runs."""

    def __getattr__(self, name):
        inner = StubLibrary.__getattr__(self, name)

        def entry(*args):
            for role, a in zip(self.roles, args[1:]):
                if a is None:
                    continue
                if role == "points":
                    self.seen[role] = _at(a, (N, 8)).copy()
                if role == "keys":
                    self.seen[role] = np.ctypeslib.as_array((ctypes.c_uint32 * (N * 4)).from_address(a)).reshape(N, 4).copy()
                if role == "layer_hits":
                    self.seen[role] = _at(a, (LAYERS, N, 8)).copy()
                if role == "incoming":
                    self.seen[role] = _at(a, (N, 3)).copy()
                if role == "sampling":
                    s = rt64.GI_SAMPLING.from_address(a)
                    self.seen[role] = (s.giSamples, s.giBounces, s.diSamples, s.flags)
            return inner(*args)
        return entry


def _keys(n=N):
    return (np.arange(n * 4, dtype=np.uint32).reshape(n, 4) * 77 + 3)


def _layer_hits():
    return np.arange(LAYERS * N * 8, dtype=np.float32).reshape(LAYERS, N, 8) + 500.0


def _incoming():
    return np.arange(N * 3, dtype=np.float32).reshape(N, 3) * 0.25


@pytest.mark.parametrize("with_keys", [False, True])
@pytest.mark.parametrize("gi_samples", [-1, 4])
@pytest.mark.parametrize("second", [False, True])
def test_gi_rays(with_keys, gi_samples, second):
    roles = ("points", "keys", "sampling", "slot", "flags", "out0", "count")
    lib = GiStub(roles=roles)
    points, keys = _rays(), (_keys() if with_keys else None)
    out = rt64.gi_rays(lib, VIEW, points, 2, keys, gi_samples, second)
    (got, args), = lib.calls
    assert got == "GenerateViewPointGIRays" and args[0] == VIEW and len(args) == 1 + len(roles)
    assert np.array_equal(lib.seen["points"], points)
    assert np.array_equal(lib.seen["keys"], keys) if with_keys else args[2] is None
    assert args[3] is None if gi_samples == -1 else lib.seen["sampling"] == (4, -1, -1, 0)
    assert args[4] == 2 and args[5] == (rt64.GI_RAYS_SECOND_BOUNCE if second else 0) and args[6] == out.ctypes.data and args[7] == N
    assert isinstance(out, np.ndarray) and out.shape == (N, 8) and out.dtype == np.float32 and out.flags["C_CONTIGUOUS"]


@pytest.mark.parametrize("with_keys", [False, True])
@pytest.mark.parametrize("with_incoming", [False, True])
@pytest.mark.parametrize("di_samples", [-1, 0, 7])
def test_shade_gi_rays(with_keys, with_incoming, di_samples):
    roles = ("rays", "layer_hits", "max_layers", "keys", "incoming", "sampling", "out0", "count")
    lib = GiStub(roles=roles)
    rays, hits, keys, incoming = _rays(), _layer_hits(), (_keys() if with_keys else None), (_incoming() if with_incoming else None)
    out = rt64.shade_gi_rays(lib, VIEW, rays, hits, keys, incoming, di_samples)
    (got, args), = lib.calls
    assert got == "ComposeViewGIRays" and args[0] == VIEW and len(args) == 1 + len(roles)
    assert np.array_equal(lib.seen["rays"], rays) and np.array_equal(lib.seen["layer_hits"], hits) and args[3] == LAYERS
    assert np.array_equal(lib.seen["keys"], keys) if with_keys else args[4] is None
    assert np.array_equal(lib.seen["incoming"], incoming) if with_incoming else args[5] is None
    assert args[6] is None if di_samples == -1 else lib.seen["sampling"] == (-1, -1, di_samples, 0)
    assert args[7] == out.ctypes.data and args[8] == N
    assert out.shape == (N, 16) and out.dtype == np.float32 and out.view(rt64.GI_SAMPLE_DTYPE).shape == (N, 1)


@pytest.mark.parametrize("with_keys", [False, True])
@pytest.mark.parametrize("overrides", [(-1, -1, -1), (3, -1, -1), (-1, 2, -1), (0, 1, 64)])
@pytest.mark.parametrize("samples", [False, True])
def test_sample_indirect(with_keys, overrides, samples):
    roles = ("points", "keys", "sampling", "samples", "out", "count")
    lib = GiStub(roles=roles)
    points, keys = _rays(), (_keys() if with_keys else None)
    if samples and overrides[0] < 0:
        with pytest.raises(ValueError) as e:
            rt64.sample_indirect(lib, VIEW, points, keys, *overrides, samples=True)
        assert str(e.value) == "samples: give gi_samples, the array is sized by it" and not lib.calls
        return
    result = rt64.sample_indirect(lib, VIEW, points, keys, *overrides, samples=samples)
    (got, args), = lib.calls
    assert got == "TraceViewPointsIndirect" and args[0] == VIEW and len(args) == 1 + len(roles)
    assert np.array_equal(lib.seen["points"], points)
    assert np.array_equal(lib.seen["keys"], keys) if with_keys else args[2] is None
    assert args[3] is None if overrides == (-1, -1, -1) else lib.seen["sampling"] == overrides + (0,)
    records = result[0] if samples else result
    assert isinstance(result, tuple) == samples and args[5] == records.ctypes.data and args[6] == N
    assert records.shape == (N, 12) and records.dtype == np.float32 and records.view(rt64.POINT_INDIRECT_DTYPE).shape == (N, 1)
    if samples and overrides[0] > 0:
        assert result[1].shape == (overrides[0], N, 16) and result[1].dtype == np.float32 and args[4] == result[1].ctypes.data
    else:
        assert args[4] is None and (not samples or result[1].shape == (0, N, 16))


@pytest.mark.parametrize("with_lods", [False, True])
@pytest.mark.parametrize("with_keys", [False, True])
def test_trace_indirect(with_lods, with_keys):
    roles = ("rays", "out0", "lods", "keys", "sampling", "out1", "count", "flags")
    lib = GiStub(roles=roles)
    rays, lods, keys = _rays(), (_lods() if with_lods else None), (_keys() if with_keys else None)
    hits, records = rt64.trace_indirect(lib, VIEW, rays, lods, keys, 2, 2, 5, flags=0x1)
    (got, args), = lib.calls
    assert got == "TraceViewRayIndirect" and args[0] == VIEW and len(args) == 1 + len(roles)
    assert np.array_equal(lib.seen["rays"], rays) and args[2] == hits.ctypes.data
    assert np.array_equal(lib.seen["lods"], lods) if with_lods else args[3] is None
    assert np.array_equal(lib.seen["keys"], keys) if with_keys else args[4] is None
    assert lib.seen["sampling"] == (2, 2, 5, 0) and args[6] == records.ctypes.data and args[7] == N and args[8] == 0x1
    assert hits.shape == (N, 8) and records.shape == (N, 12)


def test_structured_points_and_strided_inputs_are_converted():
    lib = GiStub(roles=("points", "keys", "sampling", "samples", "out", "count"))
    pts = np.zeros(N, dtype=rt64.GI_POINT_DTYPE)
    pts["position"] = np.arange(N * 3).reshape(N, 3); pts["normal"][:, 1] = 1.0; pts["instance"] = np.arange(N) - 1; pts["flags"][2] = rt64.GI_POINT_NONE
    keys = np.zeros(N, dtype=rt64.LIGHT_SAMPLE_KEY_DTYPE); keys["x"] = np.arange(N) + 70; keys["frame"] = 63
    rt64.sample_indirect(lib, VIEW, pts, keys)
    seen = lib.seen["points"]
    assert np.array_equal(seen[:, 0:3], pts["position"]) and np.array_equal(seen.view(np.int32)[:, 7], pts["instance"]) and seen.view(np.uint32)[2, 3] == rt64.GI_POINT_NONE
    assert np.array_equal(lib.seen["keys"], np.stack([keys["x"], keys["y"], keys["frame"], keys["reserved"]], axis=1))
    lib = GiStub(roles=("rays", "layer_hits", "max_layers", "keys", "incoming", "sampling", "out0", "count"))
    rays64 = np.asfortranarray(_rays().astype(np.float64))
    hits_strided = np.repeat(_layer_hits(), 2, axis=1)[:, ::2]
    incoming64 = np.repeat(_incoming().astype(np.float64), 2, axis=0)[::2]
    keys_strided = np.repeat(_keys().astype(np.int64), 2, axis=0)[::2]
    rt64.shade_gi_rays(lib, VIEW, rays64, hits_strided, keys_strided, incoming64)
    for role, want in (("rays", _rays()), ("layer_hits", _layer_hits()), ("incoming", _incoming()), ("keys", _keys())):
        assert lib.seen[role].dtype == (np.uint32 if role == "keys" else np.float32) and np.array_equal(lib.seen[role], want), role


def test_defaults_and_an_empty_batch_go_through():
    lib = StubLibrary()
    empty = np.zeros((0, 8), dtype=np.float32)
    assert rt64.sample_indirect(lib, VIEW, empty).shape == (0, 12)
    assert rt64.gi_rays(lib, VIEW, empty, 1).shape == (0, 8)
    assert rt64.shade_gi_rays(lib, VIEW, empty, np.zeros((16, 0, 8), dtype=np.float32)).shape == (0, 16)
    hits, records = rt64.trace_indirect(lib, VIEW, empty)
    assert hits.shape == (0, 8) and records.shape == (0, 12)
    assert lib.calls[0][1][2:5] == (None, None, None) and lib.calls[0][1][-1] == 0          # keys, sampling, samples = NULL; count
    assert lib.calls[1][1][2:6] == (None, None, 1, 0)                                       # keys, sampling = NULL; slot, flags
    assert lib.calls[2][1][3:7] == (16, None, None, None)                                   # maxLayers; keys, incoming, sampling = NULL
    assert lib.calls[3][1][3:6] == (None, None, None) and lib.calls[3][1][-2:] == (0, 0)    # lods, keys, sampling = NULL; count, flags


def test_wrong_shapes_raise_value_errors():
    lib = StubLibrary()
    for bad in (np.zeros((N, 7), dtype=np.float32), np.zeros((N * 8,), dtype=np.float32), np.zeros((N, 2, 4), dtype=np.float32)):
        for call in (lambda: rt64.sample_indirect(lib, VIEW, bad), lambda: rt64.gi_rays(lib, VIEW, bad, 1), lambda: rt64.trace_indirect(lib, VIEW, bad),
                     lambda: rt64.shade_gi_rays(lib, VIEW, bad, _layer_hits())):
            with pytest.raises(ValueError):
                call()
    for keys in (_keys(N + 1), _keys(N - 1), np.zeros((N, 3), dtype=np.uint32), np.zeros((N, 4), dtype=np.float32)):
        for call in (lambda: rt64.sample_indirect(lib, VIEW, _rays(), keys), lambda: rt64.gi_rays(lib, VIEW, _rays(), 1, keys), lambda: rt64.trace_indirect(lib, VIEW, _rays(), None, keys),
                     lambda: rt64.shade_gi_rays(lib, VIEW, _rays(), _layer_hits(), keys)):
            with pytest.raises(ValueError) as e:
                call()
            assert str(e.value) == KEYS
    with pytest.raises(ValueError) as e:
        rt64.trace_indirect(lib, VIEW, _rays(), _lods(N + 1))
    assert str(e.value) == LODS
    for hits, word in ((np.zeros((N, 8), dtype=np.float32), "hits: an (L, N, 8) float32 array"), (np.zeros((17, N, 8), dtype=np.float32), "max_layers: 1 to 16"),
                       (np.zeros((2, N + 1, 8), dtype=np.float32), "one list of hits per ray")):
        with pytest.raises(ValueError) as e:
            rt64.shade_gi_rays(lib, VIEW, _rays(), hits)
        assert str(e.value) == word
    with pytest.raises(ValueError) as e:
        rt64.shade_gi_rays(lib, VIEW, _rays(), _layer_hits(), None, np.zeros((N, 4), dtype=np.float32))
    assert str(e.value) == "incoming: an (N, 3) float32 array"
    assert not lib.calls          # nothing reached the library


def test_a_refusal_raises_with_the_last_error():
    lib = StubLibrary(status=0)
    for call, entry in ((lambda: rt64.sample_indirect(lib, VIEW, _rays(), _keys(), 65, 3, 65), "TraceViewPointsIndirect"), (lambda: rt64.gi_rays(lib, VIEW, _rays(), 0), "GenerateViewPointGIRays"),
                        (lambda: rt64.shade_gi_rays(lib, VIEW, _rays(), _layer_hits()), "ComposeViewGIRays"), (lambda: rt64.trace_indirect(lib, VIEW, _rays()), "TraceViewRayIndirect")):
        with pytest.raises(RuntimeError) as e:
            call()          # (out-of-range overrides and slots are the library's to refuse)
        assert str(e.value) == "stub: refused" and lib.calls[-1][0] == entry


def test_the_device_branch_refuses_cpu_tensors():
    """torch tensors select the device branch; its validation wants CUDA tensors, so CPU tensors reach the checks without a GPU."""
    torch = pytest.importorskip("torch")
    lib = StubLibrary()
    points = torch.zeros((N, 8))
    with pytest.raises(ValueError) as e:
        rt64.sample_indirect(lib, VIEW, points, torch.zeros((N, 4), dtype=torch.int32))
    assert str(e.value) == "keys: an (N, 4) int32 or uint32 CUDA tensor"
    with pytest.raises(ValueError) as e:
        rt64.sample_indirect(lib, VIEW, points)
    assert str(e.value) == ONE_ARRAY.replace("array", "CUDA tensor")
    with pytest.raises(ValueError) as e:
        rt64.shade_gi_rays(lib, VIEW, points, torch.zeros((2, N, 8)))
    assert str(e.value) == "hits: an (L, N, 8) float32 CUDA tensor"
    assert not lib.calls
