"""The boundary of the radiance calls (include/rt64_radiance.h) and their four wrappers in rt64.py, without a GPU: the header compiles on its own and after every
other header as C11 and C++17, both records have the documented sizes, offsets and flag values, the header's X-list and rt64.RADIANCE_API name the same seven
entry points with the same number of arguments, and against the stub library of tests/test_query_bindings_cpu.py each wrapper calls its entry point with its
arguments in order, allocates what it returns and refuses wrong shapes and max_layers before any library call.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import __graft_entry__ as graft
from sm64rt_legacy_renderer_amd import rt64
from test_query_bindings_cpu import LODS, N, ONE_ARRAY, VIEW, StubLibrary, _at, _lods, _rays

ROOT = graft.ROOT
HEADER = os.path.join(ROOT, "include", "rt64_radiance.h")
NAMES = ["RT64_SkyViewRays", "RT64_SkyViewRaysDevice", "RT64_SkyViewPixels", "RT64_SkyViewPixelsDevice", "RT64_ComposeViewRayRadiance",
         "RT64_ComposeViewRayRadianceDevice", "RT64_TraceViewRayRadiance"]
SKY_FIELDS, SKY_OFFSETS = ("color", "alpha", "uv", "flags", "reserved"), [0, 12, 16, 24, 28]
RADIANCE_FIELDS = ("radiance", "flags", "surface", "transmittance", "transparent", "litLayer", "light", "layers")
RADIANCE_OFFSETS = [0, 12, 16, 28, 32, 44, 48, 60]
FLAGS = [("SKY_VALID", 0x1), ("SKY_NO_TEXTURE", 0x2), ("SKY_BACKGROUND", 0x4), ("RADIANCE_VALID", 0x01), ("RADIANCE_COVERED", 0x02), ("RADIANCE_BAD_HIT", 0x04),
         ("RADIANCE_LIT", 0x08), ("RADIANCE_FOGGED", 0x10), ("RADIANCE_TRUNCATED", 0x20), ("RADIANCE_FLAG_UNSHADOWED", 0x100), ("RADIANCE_FLAG_FOG_FROM_CAMERA", 0x200)]
OTHER_HEADERS = ("rt64.h", "rt64_query.h", "rt64_surface.h", "rt64_material.h", "rt64_alpha.h", "rt64_lighting.h", "rt64_footprint.h", "rt64_bounce.h", "rt64_layers.h")
# what the other boundary tests search the exports for: none of these words may occur in a name of this list
OTHER_WORDS = r"Surface|Resolve|ShadeView|RayMaterial|Alpha|Visibility|LightView|Lighting|Footprint|CameraRays|Bounce|MirrorChain|Layers"
L = 3


def _declared():
    """(member, symbol, number of arguments) of every X(...) of RT64_RADIANCE_API_LIST."""
    body = re.search(r"#define RT64_RADIANCE_API_LIST\(X\)(.*?)\n\n", open(HEADER).read(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [(m, s, len(args.split(","))) for m, s, args in re.findall(r"X\((\w+),\s*(RT64_\w+),\s*int,\s*\(([^)]*)\)\)", body)]


PROBE = r"""
#include <stdio.h>
%s
int main(void) {
    RT64_LIBRARY lib; RT64_LIBRARY_RADIANCE p; RT64_LIBRARY_LAYERS l;
    lib.handle = 0; p = RT64_LoadLibraryRadiance(lib); l = RT64_LoadLibraryLayers(lib);
    printf("%%d %%d %%d", (int)sizeof(RT64_RAY_SKY), (int)sizeof(RT64_RAY_RADIANCE), (int)sizeof(RT64_LIBRARY_RADIANCE) / (int)sizeof(void *));
""" + "".join('    printf(" %%%%d", (int)offsetof(RT64_RAY_SKY, %s));\n' % f for f in SKY_FIELDS) + \
    "".join('    printf(" %%%%d", (int)offsetof(RT64_RAY_RADIANCE, %s));\n' % f for f in RADIANCE_FIELDS) + r"""
    printf("\n%%d %%d %%d %%d %%d %%d %%d %%d", p.SkyViewRays == 0, p.SkyViewRaysDevice == 0, p.SkyViewPixels == 0, p.SkyViewPixelsDevice == 0, p.ComposeViewRayRadiance == 0,
           p.ComposeViewRayRadianceDevice == 0, p.TraceViewRayRadiance == 0, l.TraceViewRayLayers == 0);
""" + "".join('    printf(" %%%%d", RT64_%s);\n' % n for n, _ in FLAGS) + r"""
    printf("\n");
    return 0;
}
"""
INCLUDES = {"alone": '#include "rt64_radiance.h"', "after_all": "".join('#include "%s"\n' % h for h in OTHER_HEADERS) + '#include "rt64_radiance.h"'}


@pytest.mark.parametrize("includes", sorted(INCLUDES))
@pytest.mark.parametrize("lang", ["c", "cpp"])
def test_radiance_header_compiles_and_layouts_match(tmp_path, lang, includes):
    src = tmp_path / ("probe." + lang)
    src.write_text(PROBE % INCLUDES[includes])
    exe = tmp_path / "probe"
    cc, std = ("gcc", "-std=c11") if lang == "c" else ("g++", "-std=c++17")
    subprocess.run([cc, std, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-ldl"], check=True)
    out = subprocess.run([str(exe)], stdout=subprocess.PIPE, text=True, check=True).stdout.split("\n")
    assert [int(x) for x in out[0].split()] == [32, 64, 7] + SKY_OFFSETS + RADIANCE_OFFSETS
    assert [int(x) for x in out[1].split()] == [1] * 8 + [v for _, v in FLAGS]


def test_python_binding_matches_the_radiance_list():
    declared = _declared()
    assert [s for _, s, _ in declared] == NAMES
    assert [(m, s, len(a)) for m, s, _, a in rt64.RADIANCE_API] == declared          # the same members, symbols and argument counts, in the header's order
    assert all(r is C.c_int for _, _, r, _ in rt64.RADIANCE_API)
    assert C.sizeof(rt64.RAY_SKY) == 32 and C.sizeof(rt64.RAY_RADIANCE) == 64
    assert [getattr(rt64.RAY_SKY, f).offset for f in SKY_FIELDS] == SKY_OFFSETS
    assert [getattr(rt64.RAY_RADIANCE, f).offset for f in RADIANCE_FIELDS] == RADIANCE_OFFSETS
    assert [getattr(rt64, n) for n, _ in FLAGS] == [v for _, v in FLAGS]
    # a list of its own: in no other list, in no other header, and under none of the words the other boundary tests search the exports for
    names = set(NAMES)
    assert not names & set(rt64.exported_symbols())
    for attr in ("QUERY_API", "SURFACE_API", "MATERIAL_API", "ALPHA_API", "LIGHTING_API", "FOOTPRINT_API", "BOUNCE_API", "LAYERS_API"):
        assert not names & set(s for _, s, _, _ in getattr(rt64, attr)), attr
    for other in OTHER_HEADERS:
        text = open(os.path.join(ROOT, "include", other)).read()
        assert not any(n in text for n in NAMES), other
    assert not [n for n in NAMES if re.search(OTHER_WORDS, n)]


def test_library_exports_the_radiance_list():
    lib = os.path.join(graft.PKG_DIR, "librt64.so")
    if not os.path.exists(lib):
        graft.build()
    h = C.CDLL(lib, mode=C.RTLD_LOCAL)
    for name in NAMES:
        assert hasattr(h, name), name
    exported = subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert sorted(set(re.findall(r"\bRT64_\w*(?:Radiance|SkyView)\w*", exported))) == sorted(NAMES)          # exactly the seven
    loaded = rt64.Library()
    assert all(callable(getattr(loaded, m)) for m, _, _ in _declared())


def _hits(layers=L, n=N):
    return np.arange(layers * n * 8, dtype=np.float32).reshape(layers, n, 8) + 100.0


def test_sky_wrappers_argument_order_and_outputs():
    lib = StubLibrary(roles=("rays",))
    rays = _rays()
    sky = rt64.sky_view_rays(lib, VIEW, np.asfortranarray(rays.astype(np.float64)))
    name, args = lib.calls[0]
    assert name == "SkyViewRays" and args == (VIEW, args[1], sky.ctypes.data, N) and np.array_equal(lib.seen["rays"], rays)
    assert sky.shape == (N, 8) and sky.dtype == np.float32 and sky.flags["C_CONTIGUOUS"]
    pixels = np.array([[0, 0], [63, 35], [7, 9]], dtype=np.int64)
    seen = {}

    class Lib(StubLibrary):
        def __getattr__(self, name):
            def entry(*args):
                self.calls.append((name, args))
                if args[1] is not None:
                    seen["pixels"] = np.ctypeslib.as_array((C.c_uint32 * 6).from_address(args[1])).reshape(3, 2).copy()
                return 1
            return entry
    lib = Lib()
    sky = rt64.sky_view_pixels(lib, VIEW, pixels)
    name, args = lib.calls[0]
    assert name == "SkyViewPixels" and len(args) == 4 and args[0] == VIEW and args[2] == sky.ctypes.data and args[3] == 3
    assert np.array_equal(seen["pixels"], pixels) and sky.shape == (3, 8) and sky.dtype == np.float32
    sky = rt64.sky_view_pixels(lib, VIEW, count=11)
    name, args = lib.calls[1]
    assert name == "SkyViewPixels" and args[1] is None and args[2] == sky.ctypes.data and args[3] == 11 and sky.shape == (11, 8)


@pytest.mark.parametrize("with_lods", [False, True])
def test_resolve_argument_order_and_outputs(with_lods):
    got = {}

    class Lib(StubLibrary):
        def __getattr__(self, name):
            inner = StubLibrary.__getattr__(self, name)

            def entry(*args):
                got["hits"] = _at(args[2], (L, N, 8)).copy()
                return inner(*args)
            return entry
    lib = Lib(roles=("rays", "hitlist", "lods"))
    rays, lods = _rays(), (_lods() if with_lods else None)
    flags = rt64.RADIANCE_FLAG_UNSHADOWED | rt64.RAY_FLAG_CULL_BACK_FACING
    out = rt64.resolve_view_ray_radiance(lib, VIEW, rays, np.asfortranarray(_hits().astype(np.float64)), lods, flags=flags)
    name, args = lib.calls[0]
    assert name == "ComposeViewRayRadiance" and args[0] == VIEW and len(args) == 8
    assert np.array_equal(lib.seen["rays"], rays) and (np.array_equal(lib.seen["lods"], lods) if with_lods else args[3] is None)
    assert got["hits"].dtype == np.float32 and np.array_equal(got["hits"], _hits())          # contiguous float32, layer-major
    assert isinstance(args[2], int) and args[4] == L and args[5] == out.ctypes.data and args[6:] == (N, flags)
    assert out.shape == (N, 16) and out.dtype == np.float32 and out.flags["C_CONTIGUOUS"]
    assert rt64.resolve_view_ray_radiance(lib, VIEW, rays, _hits()).shape == (N, 16) and lib.calls[1][1][-1] == 0          # flags default to 0


@pytest.mark.parametrize("hits,layers", [(True, True), (True, False), (False, True), (False, False)])
def test_trace_argument_order_and_outputs(hits, layers):
    lib = StubLibrary(roles=("rays", "lods"))
    rays, lods = _rays(), _lods()
    outs = rt64.trace_view_ray_radiance(lib, VIEW, rays, L, lods, flags=0x201, hits=hits, layers=layers)
    outs = outs if isinstance(outs, tuple) else (outs,)
    name, args = lib.calls[0]
    assert name == "TraceViewRayRadiance" and args[0] == VIEW and len(args) == 9 and args[3] == L and args[7:] == (N, 0x201)
    assert np.array_equal(lib.seen["rays"], rays) and np.array_equal(lib.seen["lods"], lods)
    assert len(outs) == 1 + hits + layers
    want = iter(outs)
    if hits:
        h = next(want); assert args[4] == h.ctypes.data and h.shape == (L, N, 8) and h.dtype == np.float32
    else:
        assert args[4] is None
    if layers:
        ly = next(want); assert args[5] == ly.ctypes.data and ly.shape == (N, 4) and ly.dtype == np.uint32
    else:
        assert args[5] is None
    r = next(want)
    assert args[6] == r.ctypes.data and r.shape == (N, 16) and r.dtype == np.float32
    full = rt64.trace_view_ray_radiance(lib, VIEW, rays)
    assert full[0].shape == (16, N, 8) and lib.calls[1][1][3] == 16 and lib.calls[1][1][2] is None and lib.calls[1][1][-1] == 0


def test_wrong_arguments_raise_value_errors_before_any_call():
    lib = StubLibrary()
    for bad in (0, 17, -1):
        with pytest.raises(ValueError) as e:
            rt64.trace_view_ray_radiance(lib, VIEW, _rays(), bad)
        assert str(e.value) == "max_layers: 1 to 16"
    with pytest.raises(ValueError) as e:
        rt64.resolve_view_ray_radiance(lib, VIEW, _rays(), _hits(17))
    assert str(e.value) == "max_layers: 1 to 16"
    for bad in (np.zeros((N, 7), dtype=np.float32), np.zeros((N * 8,), dtype=np.float32)):
        for call in (lambda: rt64.sky_view_rays(lib, VIEW, bad), lambda: rt64.trace_view_ray_radiance(lib, VIEW, bad, 4)):
            with pytest.raises(ValueError) as e:
                call()
            assert str(e.value) == ONE_ARRAY
    for lods in (np.zeros((N, 1), dtype=np.float32), _lods(N + 1)):
        for call in (lambda: rt64.trace_view_ray_radiance(lib, VIEW, _rays(), 4, lods), lambda: rt64.resolve_view_ray_radiance(lib, VIEW, _rays(), _hits(), lods)):
            with pytest.raises(ValueError) as e:
                call()
            assert str(e.value) == LODS
    for hits in (_rays(), np.zeros((L, N, 7), dtype=np.float32)):
        with pytest.raises(ValueError) as e:
            rt64.resolve_view_ray_radiance(lib, VIEW, _rays(), hits)
        assert str(e.value) == "hits: an (L, N, 8) float32 array"
    with pytest.raises(ValueError) as e:
        rt64.resolve_view_ray_radiance(lib, VIEW, _rays(), _hits(L, N + 1))
    assert str(e.value) == "one list of hits per ray"
    for pixels in (np.zeros((N, 3), dtype=np.uint32), np.zeros((N * 2,), dtype=np.uint32)):
        with pytest.raises(ValueError) as e:
            rt64.sky_view_pixels(lib, VIEW, pixels)
        assert str(e.value) == "pixels: an (N, 2) uint32 array"
    with pytest.raises(ValueError):
        rt64.sky_view_pixels(lib, VIEW)                                   # neither pixels nor a count
    with pytest.raises(ValueError):
        rt64.sky_view_pixels(lib, VIEW, np.zeros((N, 2), dtype=np.uint32), count=N)
    assert not lib.calls          # nothing reached the library


def test_a_refusal_raises_with_the_last_error_and_cpu_tensors_are_refused():
    lib = StubLibrary(status=0)
    calls = [lambda: rt64.sky_view_rays(lib, VIEW, _rays()), lambda: rt64.sky_view_pixels(lib, VIEW, count=4),
             lambda: rt64.resolve_view_ray_radiance(lib, VIEW, _rays(), _hits()), lambda: rt64.trace_view_ray_radiance(lib, VIEW, _rays(), 4)]
    for call in calls:
        with pytest.raises(RuntimeError) as e:
            call()
        assert str(e.value) == "stub: refused"
    assert [c[0] for c in lib.calls] == ["SkyViewRays", "SkyViewPixels", "ComposeViewRayRadiance", "TraceViewRayRadiance"]
    torch = pytest.importorskip("torch")
    lib = StubLibrary()
    rays, hits = torch.zeros((N, 8)), torch.zeros((L, N, 8))
    with pytest.raises(ValueError) as e:
        rt64.sky_view_rays(lib, VIEW, rays)
    assert str(e.value) == "rays: an (N, 8) float32 CUDA tensor"
    with pytest.raises(ValueError) as e:
        rt64.resolve_view_ray_radiance(lib, VIEW, rays, hits)
    assert str(e.value) == "hits: an (L, N, 8) float32 CUDA tensor"
    assert not lib.calls
