"""CPU-only checks of the boundary of the layer calls (include/rt64_layers.h): the header compiles on its own, after rt64.h and after every other header, as C11 and
C++17, the two records are 16 bytes with the documented offsets and flag values, and librt64.so / the Python binding carry exactly the names of
RT64_LAYERS_API_LIST -- in a list of their own, not in any other *_API or exported_symbols(), and in no other header."""
import ctypes as C
import os
import re
import subprocess

import pytest

import __graft_entry__ as graft

ROOT = graft.ROOT
HEADER = os.path.join(ROOT, "include", "rt64_layers.h")
NAMES = ["RT64_TraceViewRayLayers", "RT64_TraceViewRayLayersDevice", "RT64_WeighViewRayLayers", "RT64_WeighViewRayLayersDevice"]
LAYER_FIELDS = ("count", "flags", "nodesVisited", "trianglesTested")
COVERAGE_FIELDS = ("transmittance", "refraction", "shaded", "flags")
OFFSETS = [0, 4, 8, 12]
FLAGS = [("LAYERS_VALID", 0x1), ("LAYERS_ENDS_OPAQUE", 0x2), ("LAYERS_FULL", 0x4), ("COVERAGE_VALID", 0x1), ("COVERAGE_COVERED", 0x2), ("COVERAGE_GLASS", 0x4),
         ("COVERAGE_BAD_HIT", 0x8)]
OTHER_HEADERS = ("rt64.h", "rt64_query.h", "rt64_surface.h", "rt64_material.h", "rt64_alpha.h", "rt64_lighting.h", "rt64_footprint.h", "rt64_bounce.h")
OTHER_WORDS = r"Surface|Resolve|ShadeView|RayMaterial|Alpha|Visibility|LightView|Lighting|Footprint|CameraRays|Bounce|MirrorChain"          # what the other boundary tests search the exports for
# the other lists as they stand: (header, macro, Python list, number of members)
OTHER_LISTS = [("rt64_query.h", "RT64_QUERY_API_LIST", "QUERY_API", 3), ("rt64_surface.h", "RT64_SURFACE_API_LIST", "SURFACE_API", 3),
               ("rt64_material.h", "RT64_MATERIAL_API_LIST", "MATERIAL_API", 3), ("rt64_alpha.h", "RT64_ALPHA_API_LIST", "ALPHA_API", 4),
               ("rt64_lighting.h", "RT64_LIGHTING_API_LIST", "LIGHTING_API", 3), ("rt64_footprint.h", "RT64_FOOTPRINT_API_LIST", "FOOTPRINT_API", 5),
               ("rt64_bounce.h", "RT64_BOUNCE_API_LIST", "BOUNCE_API", 5)]


@pytest.fixture(scope="module")
def built():
    lib = os.path.join(graft.PKG_DIR, "librt64.so")
    if not os.path.exists(lib):
        graft.build()
    return lib


def _declared(header=HEADER, macro="RT64_LAYERS_API_LIST"):
    text = open(header).read()
    body = re.search(r"#define %s\(X\)(.*?)\n\n" % macro, text, re.S).group(1)
    return re.findall(r"X\((\w+),\s*(RT64_\w+),", body)


PROBE = r"""
#include <stdio.h>
%s
int main(void) {
    RT64_LIBRARY lib; RT64_LIBRARY_LAYERS p; RT64_LIBRARY_ALPHA a;
    lib.handle = 0; p = RT64_LoadLibraryLayers(lib); a = RT64_LoadLibraryAlpha(lib);
    printf("%%d %%d %%d %%d %%d %%d", (int)sizeof(RT64_RAY_LAYERS), (int)sizeof(RT64_RAY_COVERAGE), (int)sizeof(RT64_RAY), (int)sizeof(RT64_RAY_HIT),
           (int)sizeof(RT64_LIBRARY_LAYERS) / (int)sizeof(void *), RT64_RAY_LAYERS_MAX);
""" + "".join('    printf(" %%%%d", (int)offsetof(RT64_RAY_LAYERS, %s));\n' % f for f in LAYER_FIELDS) + \
    "".join('    printf(" %%%%d", (int)offsetof(RT64_RAY_COVERAGE, %s));\n' % f for f in COVERAGE_FIELDS) + r"""
    printf("\n%%d %%d %%d %%d %%d", p.TraceViewRayLayers == 0, p.TraceViewRayLayersDevice == 0, p.WeighViewRayLayers == 0, p.WeighViewRayLayersDevice == 0, a.TraceViewRaysAlpha == 0);
""" + "".join('    printf(" %%%%d", RT64_%s);\n' % n for n, _ in FLAGS) + r"""
    printf("\n");
    return 0;
}
"""
INCLUDES = {"alone": '#include "rt64_layers.h"', "after_all": "".join('#include "%s"\n' % h for h in OTHER_HEADERS) + '#include "rt64_layers.h"'}
INCLUDES.update({"after_" + h[:-2]: '#include "%s"\n#include "rt64_layers.h"' % h for h in OTHER_HEADERS})


@pytest.mark.parametrize("includes", sorted(INCLUDES))
@pytest.mark.parametrize("lang", ["c", "cpp"])
def test_layers_header_compiles_and_layouts_match(tmp_path, lang, includes):
    src = tmp_path / ("probe." + lang)
    src.write_text(PROBE % INCLUDES[includes])
    exe = tmp_path / "probe"
    cc, std = ("gcc", "-std=c11") if lang == "c" else ("g++", "-std=c++17")
    subprocess.run([cc, std, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-ldl"], check=True)
    out = subprocess.run([str(exe)], stdout=subprocess.PIPE, text=True, check=True).stdout.split("\n")
    assert [int(x) for x in out[0].split()] == [16, 16, 32, 32, 4, 16] + OFFSETS + OFFSETS
    assert [int(x) for x in out[1].split()] == [1] * 5 + [v for _, v in FLAGS]


def test_library_exports_the_layers_list(built):
    h = C.CDLL(built, mode=C.RTLD_LOCAL)
    declared = _declared()
    assert [s for _, s in declared] == NAMES
    for _, name in declared:
        assert hasattr(h, name), name
    exported = subprocess.run(["nm", "-D", "--defined-only", built], stdout=subprocess.PIPE, text=True, check=True).stdout
    found = sorted(set(re.findall(r"\bRT64_\w*Layers\w*", exported)))
    assert found == sorted(NAMES)                       # exactly the four: no other export with that word
    assert not [n for n in NAMES if re.search(OTHER_WORDS, n)]


def test_python_binding_matches_the_layers_list():
    from sm64rt_legacy_renderer_amd import rt64
    assert [(m, s) for m, s, _, _ in rt64.LAYERS_API] == _declared()
    assert C.sizeof(rt64.RAY_LAYERS) == 16 and C.sizeof(rt64.RAY_COVERAGE) == 16
    assert [getattr(rt64.RAY_LAYERS, f).offset for f in LAYER_FIELDS] == OFFSETS and [getattr(rt64.RAY_COVERAGE, f).offset for f in COVERAGE_FIELDS] == OFFSETS
    assert [getattr(rt64, n) for n, _ in FLAGS] == [v for _, v in FLAGS]
    assert rt64.RAY_LAYERS_MAX == 16
    # the other lists stay what they are, and the other headers do not name these functions
    names = set(NAMES)
    assert not names & set(rt64.exported_symbols())
    for header, macro, attr, count in OTHER_LISTS:
        theirs = _declared(os.path.join(ROOT, "include", header), macro)
        assert len(theirs) == count and [(m, s) for m, s, _, _ in getattr(rt64, attr)] == theirs, header
        assert not names & set(s for _, s in theirs)
    for other in OTHER_HEADERS:
        text = open(os.path.join(ROOT, "include", other)).read()
        assert not any(n in text for n in NAMES) and "Layers" not in text, other
    lib = rt64.Library()
    assert all(callable(getattr(lib, m)) for m, _ in _declared())
