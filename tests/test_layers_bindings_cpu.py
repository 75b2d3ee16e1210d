"""The two layer wrappers of rt64.py (trace_view_ray_layers, weigh_view_ray_layers) against the stub library of tests/test_query_bindings_cpu.py: which entry point
each calls, with which arguments in which order, what it allocates, what it converts, what it refuses and with which words.  No GPU and no librt64.so.
"""
import numpy as np
import pytest

from sm64rt_legacy_renderer_amd import rt64
from test_query_bindings_cpu import LODS, N, ONE_ARRAY, VIEW, StubLibrary, _at, _lods, _rays

L = 3


def _hits(layers=L, n=N):
    return np.arange(layers * n * 8, dtype=np.float32).reshape(layers, n, 8) + 100.0


@pytest.mark.parametrize("with_lods", [False, True])
@pytest.mark.parametrize("weights", [False, True])
def test_trace_argument_order_and_outputs(with_lods, weights):
    lib = StubLibrary(roles=("rays", "lods"))
    rays, lods = _rays(), (_lods() if with_lods else None)
    outs = rt64.trace_view_ray_layers(lib, VIEW, rays, L, lods, flags=0x1, weights=weights)
    assert len(lib.calls) == 1 and len(outs) == (4 if weights else 2)
    name, args = lib.calls[0]
    assert name == "TraceViewRayLayers" and args[0] == VIEW and len(args) == 10
    assert np.array_equal(lib.seen["rays"], rays) and (np.array_equal(lib.seen["lods"], lods) if with_lods else args[2] is None)
    assert args[3] == L and args[4] == outs[0].ctypes.data and args[5] == outs[1].ctypes.data and args[8:] == (N, 0x1)
    assert outs[0].shape == (L, N, 8) and outs[0].dtype == np.float32 and outs[1].shape == (N, 4) and outs[1].dtype == np.uint32
    if weights:
        assert args[6] == outs[2].ctypes.data and args[7] == outs[3].ctypes.data
        assert outs[2].shape == (L, N) and outs[2].dtype == np.float32 and outs[3].shape == (N, 4) and outs[3].dtype == np.float32
    else:
        assert args[6] is None and args[7] is None
    assert all(o.flags["C_CONTIGUOUS"] for o in outs)


@pytest.mark.parametrize("with_lods", [False, True])
def test_weigh_argument_order_and_outputs(with_lods):
    lib = StubLibrary(roles=("rays", "hitlist", "lods"))
    rays, hits, lods = _rays(), _hits(), (_lods() if with_lods else None)
    weights, coverage = rt64.weigh_view_ray_layers(lib, VIEW, rays, np.asfortranarray(hits.astype(np.float64)), lods)
    name, args = lib.calls[0]
    assert name == "WeighViewRayLayers" and args[0] == VIEW and len(args) == 8
    assert np.array_equal(lib.seen["rays"], rays) and (np.array_equal(lib.seen["lods"], lods) if with_lods else args[3] is None)
    assert isinstance(args[2], int) and args[4] == L and args[5] == weights.ctypes.data and args[6] == coverage.ctypes.data and args[7] == N
    assert weights.shape == (L, N) and weights.dtype == np.float32 and coverage.shape == (N, 4) and coverage.dtype == np.float32


def test_the_hits_reach_the_library_contiguous_float32():
    got = {}

    class Lib(StubLibrary):
        def __getattr__(self, name):
            def entry(*args):
                got["hits"] = _at(args[2], (L, N, 8)).copy()
                return 1
            return entry
    rt64.weigh_view_ray_layers(Lib(), VIEW, _rays(), np.asfortranarray(_hits().astype(np.float64)))
    assert got["hits"].dtype == np.float32 and np.array_equal(got["hits"], _hits())


def test_constants_and_an_empty_batch():
    assert (rt64.LAYERS_VALID, rt64.LAYERS_ENDS_OPAQUE, rt64.LAYERS_FULL) == (1, 2, 4)
    assert (rt64.COVERAGE_VALID, rt64.COVERAGE_COVERED, rt64.COVERAGE_GLASS, rt64.COVERAGE_BAD_HIT) == (1, 2, 4, 8) and rt64.RAY_LAYERS_MAX == 16
    lib = StubLibrary()
    empty = np.zeros((0, 8), dtype=np.float32)
    hits, layers = rt64.trace_view_ray_layers(lib, VIEW, empty, 16)
    assert hits.shape == (16, 0, 8) and layers.shape == (0, 4) and lib.calls[0][1][3] == 16 and lib.calls[0][1][-2:] == (0, 0)
    w, c = rt64.weigh_view_ray_layers(lib, VIEW, empty, hits)
    assert w.shape == (16, 0) and c.shape == (0, 4) and lib.calls[1][1][-1] == 0


def test_wrong_arguments_raise_value_errors():
    lib = StubLibrary()
    for bad in (0, 17, -1):
        with pytest.raises(ValueError) as e:
            rt64.trace_view_ray_layers(lib, VIEW, _rays(), bad)
        assert str(e.value) == "max_layers: 1 to 16"
    for bad in (np.zeros((N, 7), dtype=np.float32), np.zeros((N * 8,), dtype=np.float32)):
        with pytest.raises(ValueError) as e:
            rt64.trace_view_ray_layers(lib, VIEW, bad, 4)
        assert str(e.value) == ONE_ARRAY
    for lods in (np.zeros((N, 1), dtype=np.float32), _lods(N + 1)):
        with pytest.raises(ValueError) as e:
            rt64.trace_view_ray_layers(lib, VIEW, _rays(), 4, lods)
        assert str(e.value) == LODS
        with pytest.raises(ValueError) as e:
            rt64.weigh_view_ray_layers(lib, VIEW, _rays(), _hits(), lods)
        assert str(e.value) == LODS
    for hits in (_rays(), np.zeros((L, N, 7), dtype=np.float32)):
        with pytest.raises(ValueError) as e:
            rt64.weigh_view_ray_layers(lib, VIEW, _rays(), hits)
        assert str(e.value) == "hits: an (L, N, 8) float32 array"
    with pytest.raises(ValueError) as e:
        rt64.weigh_view_ray_layers(lib, VIEW, _rays(), _hits(L, N + 1))
    assert str(e.value) == "one list of hits per ray"
    with pytest.raises(ValueError) as e:
        rt64.weigh_view_ray_layers(lib, VIEW, _rays(), _hits(17))
    assert str(e.value) == "max_layers: 1 to 16"
    assert not lib.calls          # nothing reached the library


def test_a_refusal_raises_with_the_last_error():
    lib = StubLibrary(status=0)
    with pytest.raises(RuntimeError) as e:
        rt64.trace_view_ray_layers(lib, VIEW, _rays(), 4, weights=True)
    assert str(e.value) == "stub: refused"
    with pytest.raises(RuntimeError) as e:
        rt64.weigh_view_ray_layers(lib, VIEW, _rays(), _hits())
    assert str(e.value) == "stub: refused" and [c[0] for c in lib.calls] == ["TraceViewRayLayers", "WeighViewRayLayers"]


def test_the_device_branch_refuses_cpu_tensors():
    torch = pytest.importorskip("torch")
    lib = StubLibrary()
    rays, hits = torch.zeros((N, 8)), torch.zeros((L, N, 8))
    with pytest.raises(ValueError) as e:
        rt64.trace_view_ray_layers(lib, VIEW, rays, 4)
    assert str(e.value) == "rays: an (N, 8) float32 CUDA tensor"
    with pytest.raises(ValueError) as e:
        rt64.weigh_view_ray_layers(lib, VIEW, rays, hits)
    assert str(e.value) == "hits: an (L, N, 8) float32 CUDA tensor"
    assert not lib.calls
