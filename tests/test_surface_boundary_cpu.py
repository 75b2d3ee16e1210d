"""CPU-only checks of the surface-record boundary (include/rt64_surface.h): the header compiles on its own and after rt64.h / rt64_query.h, the record is
64 bytes with the documented offsets, and librt64.so / the Python binding carry exactly the names of RT64_SURFACE_API_LIST -- in a list of their own, not in
RT64_QUERY_API_LIST, QUERY_API or exported_symbols()."""
import ctypes as C
import os
import re
import subprocess

import pytest

import __graft_entry__ as graft

ROOT = graft.ROOT
HEADER = os.path.join(ROOT, "include", "rt64_surface.h")
NAMES = ["RT64_ResolveViewRayHits", "RT64_ResolveViewRayHitsDevice", "RT64_TraceViewRaySurfaces"]


@pytest.fixture(scope="module")
def built():
    lib = os.path.join(graft.PKG_DIR, "librt64.so")
    if not os.path.exists(lib):
        graft.build()
    return lib


def _declared():
    text = open(HEADER).read()
    body = re.search(r"#define RT64_SURFACE_API_LIST\(X\)(.*?)\n\n", text, re.S).group(1)
    return re.findall(r"X\((\w+),\s*(RT64_\w+),", body)


PROBE = r"""
#include <stdio.h>
%s
int main(void) {
    RT64_LIBRARY lib; RT64_LIBRARY_SURFACE q; RT64_LIBRARY_QUERY r;
    lib.handle = 0; q = RT64_LoadLibrarySurface(lib); r = RT64_LoadLibraryQuery(lib);
    printf("%%d %%d %%d %%d %%d %%d %%d %%d %%d %%d\n", (int)sizeof(RT64_RAY_SURFACE), (int)offsetof(RT64_RAY_SURFACE, position), (int)offsetof(RT64_RAY_SURFACE, flags),
           (int)offsetof(RT64_RAY_SURFACE, geometricNormal), (int)offsetof(RT64_RAY_SURFACE, instance), (int)offsetof(RT64_RAY_SURFACE, shadingNormal),
           (int)offsetof(RT64_RAY_SURFACE, primitive), (int)offsetof(RT64_RAY_SURFACE, uv), (int)offsetof(RT64_RAY_SURFACE, t), (int)offsetof(RT64_RAY_SURFACE, reserved));
    printf("%%d %%d %%d %%d %%d %%d %%d %%d\n", q.ResolveViewRayHits == 0, q.ResolveViewRayHitsDevice == 0, q.TraceViewRaySurfaces == 0, r.TraceViewRays == 0,
           RT64_SURFACE_VALID, RT64_SURFACE_BACK_FACE, RT64_SURFACE_HAS_UV, RT64_SURFACE_BAD_HIT);
    return 0;
}
"""
INCLUDES = {
    "alone": '#include "rt64_surface.h"',
    "after_rt64": '#include "rt64.h"\n#include "rt64_surface.h"',
    "after_query": '#include "rt64.h"\n#include "rt64_query.h"\n#include "rt64_surface.h"',
}


@pytest.mark.parametrize("includes", sorted(INCLUDES))
@pytest.mark.parametrize("lang", ["c", "cpp"])
def test_surface_header_compiles_and_layouts_match(tmp_path, lang, includes):
    src = tmp_path / ("probe." + lang)
    src.write_text(PROBE % INCLUDES[includes])
    exe = tmp_path / "probe"
    cc, std = ("gcc", "-std=c11") if lang == "c" else ("g++", "-std=c++17")
    subprocess.run([cc, std, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-ldl"], check=True)
    out = subprocess.run([str(exe)], stdout=subprocess.PIPE, text=True, check=True).stdout.split("\n")
    assert [int(x) for x in out[0].split()] == [64, 0, 12, 16, 28, 32, 44, 48, 56, 60]
    assert [int(x) for x in out[1].split()] == [1, 1, 1, 1, 1, 2, 4, 8]


def test_library_exports_the_surface_list(built):
    h = C.CDLL(built, mode=C.RTLD_LOCAL)
    declared = _declared()
    assert [s for _, s in declared] == NAMES
    for _, name in declared:
        assert hasattr(h, name), name
    exported = subprocess.run(["nm", "-D", "--defined-only", built], stdout=subprocess.PIPE, text=True, check=True).stdout
    found = sorted(set(re.findall(r"\bRT64_\w*(?:Surface|Resolve)\w*", exported)))
    assert found == sorted(NAMES)                       # exactly the three: no other surface / resolve export


def test_python_binding_matches_the_surface_list():
    from sm64rt_legacy_renderer_amd import rt64
    assert [(m, s) for m, s, _, _ in rt64.SURFACE_API] == _declared()
    assert C.sizeof(rt64.RAY_SURFACE) == 64
    assert [getattr(rt64.RAY_SURFACE, f).offset for f in ("position", "flags", "geometricNormal", "instance", "shadingNormal", "primitive", "uv", "t", "reserved")] == \
        [0, 12, 16, 28, 32, 44, 48, 56, 60]
    assert (rt64.SURFACE_VALID, rt64.SURFACE_BACK_FACE, rt64.SURFACE_HAS_UV, rt64.SURFACE_BAD_HIT) == (1, 2, 4, 8)
    # the other lists stay what they are
    names = set(NAMES)
    assert not names & set(rt64.exported_symbols())
    assert not names & set(s for _, s, _, _ in rt64.QUERY_API)
    query_header = open(os.path.join(ROOT, "include", "rt64_query.h")).read()
    assert not any(n in query_header for n in NAMES)
