"""The three footprint wrappers of rt64.py (camera_rays, footprint_hits, trace_pixel_footprints) against the stub library of tests/test_query_bindings_cpu.py:
which entry point each calls, with which arguments in which order, what it allocates, what it converts, what it refuses and with which words.  No GPU and no
librt64.so.
"""
import ctypes

import numpy as np
import pytest

from sm64rt_legacy_renderer_amd import rt64
from test_query_bindings_cpu import N, TWO_ARRAYS, VIEW, StubLibrary, _at, _rays


def _pixels(n=N):
    return np.arange(2 * n, dtype=np.uint32).reshape(n, 2)


def _diffs(n=N):
    return np.arange(n * 16, dtype=np.float32).reshape(n, 16) + 1000.0


def _pixels_at(address, n=N):
    return np.ctypeslib.as_array((ctypes.c_uint32 * (2 * n)).from_address(address)).reshape(n, 2).copy()


def test_camera_rays_argument_order_and_outputs():
    lib = StubLibrary()
    rays, diffs = rt64.camera_rays(lib, VIEW, _pixels())
    name, args = lib.calls[0]
    assert name == "GenerateViewCameraRays" and args[0] == VIEW and len(args) == 5
    assert args[2] == rays.ctypes.data and args[3] == diffs.ctypes.data and args[4] == N
    for a, w in ((rays, 8), (diffs, 16)):
        assert isinstance(a, np.ndarray) and a.shape == (N, w) and a.dtype == np.float32 and a.flags["C_CONTIGUOUS"]
    only = rt64.camera_rays(lib, VIEW, _pixels(), differentials=False)          # rays alone: diffs = NULL, one array back
    assert isinstance(only, np.ndarray) and only.shape == (N, 8) and lib.calls[1][1][3] is None and lib.calls[1][1][2] == only.ctypes.data
    rays, diffs = rt64.camera_rays(lib, VIEW, None, count=7)                     # pixels = NULL: the count is the caller's
    assert lib.calls[2][1][1] is None and lib.calls[2][1][4] == 7 and rays.shape == (7, 8) and diffs.shape == (7, 16)
    assert rt64.camera_rays(lib, VIEW, np.zeros((0, 2), dtype=np.uint32))[0].shape == (0, 8)


def test_pixels_are_made_contiguous_uint32():
    seen = {}

    class Lib(StubLibrary):
        def __getattr__(self, name):
            def entry(*args):
                seen["pixels"] = _pixels_at(args[1])
                self.calls.append((name, args))
                return 1
            return entry
    lib = Lib()
    strided = np.repeat(_pixels().astype(np.int64), 2, axis=0)[::2]          # int64, every other row of a larger array
    rt64.camera_rays(lib, VIEW, strided)
    assert np.array_equal(seen["pixels"], _pixels())
    rt64.trace_pixel_footprints(lib, VIEW, np.asfortranarray(_pixels().astype(np.float64)))
    assert np.array_equal(seen["pixels"], _pixels())


def test_trace_pixel_footprints_argument_order_and_outputs():
    lib = StubLibrary()
    rays, hits, foot = rt64.trace_pixel_footprints(lib, VIEW, _pixels(), flags=rt64.RAY_FLAG_CULL_BACK_FACING)
    name, args = lib.calls[0]
    assert name == "TraceViewPixelFootprints" and args[0] == VIEW and len(args) == 7
    assert args[2:] == (rays.ctypes.data, hits.ctypes.data, foot.ctypes.data, N, rt64.RAY_FLAG_CULL_BACK_FACING)
    assert rays.shape == (N, 8) and hits.shape == (N, 8) and foot.shape == (N, 16) and all(a.dtype == np.float32 for a in (rays, hits, foot))
    rt64.trace_pixel_footprints(lib, VIEW, None, count=3)
    assert lib.calls[1][1][1] is None and lib.calls[1][1][-2:] == (3, 0)          # pixels = NULL; count, default flags 0


@pytest.mark.parametrize("with_diffs", [False, True])
def test_footprint_hits_argument_order_and_outputs(with_diffs):
    rays, hits, diffs = _rays(), _rays() + 100.0, (_diffs() if with_diffs else None)
    seen = {}

    class Lib(StubLibrary):
        def __getattr__(self, name):
            def entry(*args):
                seen["rays"], seen["hits"] = _at(args[1], (N, 8)).copy(), _at(args[3], (N, 8)).copy()
                seen["diffs"] = _at(args[2], (N, 16)).copy() if args[2] is not None else None
                self.calls.append((name, args))
                return 1
            return entry
    lib = Lib()
    strided_hits = np.repeat(hits, 2, axis=0)[::2]
    out = rt64.footprint_hits(lib, VIEW, np.asfortranarray(rays.astype(np.float64)), diffs.astype(np.float64) if with_diffs else None, strided_hits)
    name, args = lib.calls[0]
    assert name == "FootprintViewRayHits" and args[0] == VIEW and len(args) == 6 and args[4] == out.ctypes.data and args[5] == N
    assert np.array_equal(seen["rays"], rays) and np.array_equal(seen["hits"], hits)
    assert np.array_equal(seen["diffs"], diffs) if with_diffs else (seen["diffs"] is None and args[2] is None)
    assert out.shape == (N, 16) and out.dtype == np.float32 and out.flags["C_CONTIGUOUS"]


def test_wrong_shapes_raise_value_errors():
    lib = StubLibrary()
    for bad in (np.zeros((N, 3), dtype=np.uint32), np.zeros((2 * N,), dtype=np.uint32), np.zeros((N, 2, 1), dtype=np.uint32)):
        for call in (lambda p: rt64.camera_rays(lib, VIEW, p), lambda p: rt64.trace_pixel_footprints(lib, VIEW, p)):
            with pytest.raises(ValueError) as e:
                call(bad)
            assert str(e.value) == "pixels: an (N, 2) uint32 array"
    with pytest.raises(ValueError) as e:
        rt64.camera_rays(lib, VIEW, None)
    assert str(e.value) == "pixels=None needs a count"
    with pytest.raises(ValueError) as e:
        rt64.camera_rays(lib, VIEW, _pixels(), count=N)
    assert str(e.value) == "count goes with pixels=None only"
    for hits in (_rays(N + 1), np.zeros((N, 7), dtype=np.float32)):
        with pytest.raises(ValueError) as e:
            rt64.footprint_hits(lib, VIEW, _rays(), None, hits)
        assert str(e.value) == TWO_ARRAYS
    for diffs in (_diffs(N + 1), np.zeros((N, 8), dtype=np.float32), np.zeros((N * 16,), dtype=np.float32)):
        with pytest.raises(ValueError) as e:
            rt64.footprint_hits(lib, VIEW, _rays(), diffs, _rays())
        assert str(e.value) == "diffs: an (N, 16) float32 array"
    assert not lib.calls          # nothing reached the library


def test_a_refusal_raises_with_the_last_error():
    lib = StubLibrary(status=0)
    for k, call in enumerate((lambda: rt64.camera_rays(lib, VIEW, _pixels()), lambda: rt64.footprint_hits(lib, VIEW, _rays(), _diffs(), _rays()),
                              lambda: rt64.trace_pixel_footprints(lib, VIEW, _pixels()))):
        with pytest.raises(RuntimeError) as e:
            call()
        assert str(e.value) == "stub: refused" and len(lib.calls) == k + 1
    assert [c[0] for c in lib.calls] == ["GenerateViewCameraRays", "FootprintViewRayHits", "TraceViewPixelFootprints"]


def test_the_device_branch_refuses_cpu_tensors():
    """torch tensors select the device branch; its validation wants CUDA tensors, so CPU tensors reach the check without a GPU."""
    torch = pytest.importorskip("torch")
    lib = StubLibrary()
    with pytest.raises(ValueError) as e:
        rt64.camera_rays(lib, VIEW, torch.zeros((N, 2), dtype=torch.int32))
    assert str(e.value) == "pixels: an (N, 2) uint32 / int32 CUDA tensor"
    with pytest.raises(ValueError) as e:
        rt64.footprint_hits(lib, VIEW, torch.zeros((N, 8)), torch.zeros((N, 16)), torch.zeros((N, 8)))
    assert str(e.value) == "rays, hits: (N, 8) float32 CUDA tensors"
    assert not lib.calls
