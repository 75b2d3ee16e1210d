"""CPU-only checks of the boundary of the direct-light records (include/rt64_lighting.h): the header compiles on its own and after rt64.h, as C11 and C++17, the
record is 64 bytes with the documented offsets and flag values, and librt64.so / the Python binding carry exactly the names of RT64_LIGHTING_API_LIST -- in a
list of their own, not in QUERY_API, SURFACE_API, MATERIAL_API, ALPHA_API or exported_symbols()."""
import ctypes as C
import os
import re
import subprocess

import pytest

import __graft_entry__ as graft

ROOT = graft.ROOT
HEADER = os.path.join(ROOT, "include", "rt64_lighting.h")
NAMES = ["RT64_LightViewRayHits", "RT64_LightViewRayHitsDevice", "RT64_TraceViewRayLighting"]
FIELDS = ("direct", "flags", "unshadowed", "lightsAdmitted", "emitted", "lightsBlocked", "instance", "primitive", "nodesVisited", "trianglesTested")
OFFSETS = [0, 12, 16, 28, 32, 44, 48, 52, 56, 60]
FLAGS = [("VALID", 0x01), ("BAD_HIT", 0x02), ("BACK_FACE", 0x04), ("UNLIT", 0x08), ("TRUNCATED", 0x10)]


@pytest.fixture(scope="module")
def built():
    lib = os.path.join(graft.PKG_DIR, "librt64.so")
    if not os.path.exists(lib):
        graft.build()
    return lib


def _declared():
    text = open(HEADER).read()
    body = re.search(r"#define RT64_LIGHTING_API_LIST\(X\)(.*?)\n\n", text, re.S).group(1)
    return re.findall(r"X\((\w+),\s*(RT64_\w+),", body)


PROBE = r"""
#include <stdio.h>
%s
int main(void) {
    RT64_LIBRARY lib; RT64_LIBRARY_LIGHTING p; RT64_LIBRARY_ALPHA a; RT64_LIBRARY_MATERIAL q;
    lib.handle = 0; p = RT64_LoadLibraryLighting(lib); a = RT64_LoadLibraryAlpha(lib); q = RT64_LoadLibraryMaterial(lib);
    printf("%%d %%d %%d", (int)sizeof(RT64_RAY_LIGHTING), (int)sizeof(RT64_RAY_HIT), (int)sizeof(RT64_LIBRARY_LIGHTING) / (int)sizeof(void *));
""" + "".join('    printf(" %%%%d", (int)offsetof(RT64_RAY_LIGHTING, %s));\n' % f for f in FIELDS) + r"""
    printf("\n%%d %%d %%d %%d %%d", p.LightViewRayHits == 0, p.LightViewRayHitsDevice == 0, p.TraceViewRayLighting == 0, a.TraceViewRayVisibility == 0, q.ShadeViewRayHits == 0);
""" + "".join('    printf(" %%%%d", RT64_LIGHTING_%s);\n' % n for n, _ in FLAGS) + r"""
    printf("\n");
    return 0;
}
"""
INCLUDES = {
    "alone": '#include "rt64_lighting.h"',
    "after_rt64": '#include "rt64.h"\n#include "rt64_lighting.h"',
    "after_alpha": '#include "rt64.h"\n#include "rt64_query.h"\n#include "rt64_surface.h"\n#include "rt64_material.h"\n#include "rt64_alpha.h"\n#include "rt64_lighting.h"',
}


@pytest.mark.parametrize("includes", sorted(INCLUDES))
@pytest.mark.parametrize("lang", ["c", "cpp"])
def test_lighting_header_compiles_and_layouts_match(tmp_path, lang, includes):
    src = tmp_path / ("probe." + lang)
    src.write_text(PROBE % INCLUDES[includes])
    exe = tmp_path / "probe"
    cc, std = ("gcc", "-std=c11") if lang == "c" else ("g++", "-std=c++17")
    subprocess.run([cc, std, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-ldl"], check=True)
    out = subprocess.run([str(exe)], stdout=subprocess.PIPE, text=True, check=True).stdout.split("\n")
    assert [int(x) for x in out[0].split()] == [64, 32, 3] + OFFSETS
    assert [int(x) for x in out[1].split()] == [1] * 5 + [v for _, v in FLAGS]


def test_library_exports_the_lighting_list(built):
    h = C.CDLL(built, mode=C.RTLD_LOCAL)
    declared = _declared()
    assert [s for _, s in declared] == NAMES
    for _, name in declared:
        assert hasattr(h, name), name
    exported = subprocess.run(["nm", "-D", "--defined-only", built], stdout=subprocess.PIPE, text=True, check=True).stdout
    found = sorted(set(re.findall(r"\bRT64_\w*(?:LightView|Lighting)\w*", exported)))
    assert found == sorted(NAMES)                       # exactly the three: no other export with those words


def test_python_binding_matches_the_lighting_list():
    from sm64rt_legacy_renderer_amd import rt64
    assert [(m, s) for m, s, _, _ in rt64.LIGHTING_API] == _declared()
    assert C.sizeof(rt64.RAY_LIGHTING) == 64
    assert [getattr(rt64.RAY_LIGHTING, f).offset for f in FIELDS] == OFFSETS
    assert [getattr(rt64, "LIGHTING_" + n) for n, _ in FLAGS] == [v for _, v in FLAGS]
    # the other lists stay what they are, and the headers in front of this one do not name its functions
    names = set(NAMES)
    assert not names & set(rt64.exported_symbols())
    for other in (rt64.QUERY_API, rt64.SURFACE_API, rt64.MATERIAL_API, rt64.ALPHA_API):
        assert not names & set(s for _, s, _, _ in other)
    for other in ("rt64.h", "rt64_query.h", "rt64_surface.h", "rt64_material.h", "rt64_alpha.h"):
        text = open(os.path.join(ROOT, "include", other)).read()
        assert not any(n in text for n in NAMES), other
    lib = rt64.Library()
    assert all(callable(getattr(lib, m)) for m, _ in _declared())
