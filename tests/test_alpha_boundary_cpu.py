"""CPU-only checks of the boundary of the walks that honour alpha (include/rt64_alpha.h): the header compiles on its own and after each of the headers before it,
the visibility record is 16 bytes with the documented offsets and flag values, and librt64.so / the Python binding carry exactly the names of RT64_ALPHA_API_LIST
-- in a list of their own, not in QUERY_API, SURFACE_API, MATERIAL_API or exported_symbols()."""
import ctypes as C
import os
import re
import subprocess

import pytest

import __graft_entry__ as graft

ROOT = graft.ROOT
HEADER = os.path.join(ROOT, "include", "rt64_alpha.h")
NAMES = ["RT64_TraceViewRaysAlpha", "RT64_TraceViewRaysAlphaDevice", "RT64_TraceViewRayVisibility", "RT64_TraceViewRayVisibilityDevice"]
FIELDS = ("visibility", "flags", "nodesVisited", "trianglesTested")
OFFSETS = [0, 4, 8, 12]
FLAGS = [("VALID", 0x1), ("BLOCKED", 0x2)]


@pytest.fixture(scope="module")
def built():
    lib = os.path.join(graft.PKG_DIR, "librt64.so")
    if not os.path.exists(lib):
        graft.build()
    return lib


def _declared():
    text = open(HEADER).read()
    body = re.search(r"#define RT64_ALPHA_API_LIST\(X\)(.*?)\n\n", text, re.S).group(1)
    return re.findall(r"X\((\w+),\s*(RT64_\w+),", body)


PROBE = r"""
#include <stdio.h>
%s
int main(void) {
    RT64_LIBRARY lib; RT64_LIBRARY_ALPHA a; RT64_LIBRARY_MATERIAL q; RT64_LIBRARY_SURFACE s; RT64_LIBRARY_QUERY r;
    lib.handle = 0; a = RT64_LoadLibraryAlpha(lib); q = RT64_LoadLibraryMaterial(lib); s = RT64_LoadLibrarySurface(lib); r = RT64_LoadLibraryQuery(lib);
    printf("%%d %%d", (int)sizeof(RT64_RAY_VISIBILITY), (int)sizeof(RT64_RAY_HIT));
""" + "".join('    printf(" %%%%d", (int)offsetof(RT64_RAY_VISIBILITY, %s));\n' % f for f in FIELDS) + r"""
    printf("\n%%d %%d %%d %%d %%d %%d %%d", a.TraceViewRaysAlpha == 0, a.TraceViewRaysAlphaDevice == 0, a.TraceViewRayVisibility == 0, a.TraceViewRayVisibilityDevice == 0,
           q.ShadeViewRayHits == 0, s.ResolveViewRayHits == 0, r.TraceViewRays == 0);
""" + "".join('    printf(" %%%%d", RT64_VISIBILITY_%s);\n' % n for n, _ in FLAGS) + r"""
    printf("\n");
    return 0;
}
"""
INCLUDES = {
    "alone": '#include "rt64_alpha.h"',
    "after_rt64": '#include "rt64.h"\n#include "rt64_alpha.h"',
    "after_material": '#include "rt64.h"\n#include "rt64_query.h"\n#include "rt64_surface.h"\n#include "rt64_material.h"\n#include "rt64_alpha.h"',
}


@pytest.mark.parametrize("includes", sorted(INCLUDES))
@pytest.mark.parametrize("lang", ["c", "cpp"])
def test_alpha_header_compiles_and_layouts_match(tmp_path, lang, includes):
    src = tmp_path / ("probe." + lang)
    src.write_text(PROBE % INCLUDES[includes])
    exe = tmp_path / "probe"
    cc, std = ("gcc", "-std=c11") if lang == "c" else ("g++", "-std=c++17")
    subprocess.run([cc, std, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-ldl"], check=True)
    out = subprocess.run([str(exe)], stdout=subprocess.PIPE, text=True, check=True).stdout.split("\n")
    assert [int(x) for x in out[0].split()] == [16, 32] + OFFSETS
    assert [int(x) for x in out[1].split()] == [1] * 7 + [v for _, v in FLAGS]


def test_library_exports_the_alpha_list(built):
    h = C.CDLL(built, mode=C.RTLD_LOCAL)
    declared = _declared()
    assert [s for _, s in declared] == NAMES
    for _, name in declared:
        assert hasattr(h, name), name
    exported = subprocess.run(["nm", "-D", "--defined-only", built], stdout=subprocess.PIPE, text=True, check=True).stdout
    found = sorted(set(re.findall(r"\bRT64_\w*(?:Alpha|Visibility)\w*", exported)))
    assert found == sorted(NAMES)                       # exactly the four: no other export with those words


def test_python_binding_matches_the_alpha_list():
    from sm64rt_legacy_renderer_amd import rt64
    assert [(m, s) for m, s, _, _ in rt64.ALPHA_API] == _declared()
    assert C.sizeof(rt64.RAY_VISIBILITY) == 16
    assert [getattr(rt64.RAY_VISIBILITY, f).offset for f in FIELDS] == OFFSETS
    assert [getattr(rt64, "VISIBILITY_" + n) for n, _ in FLAGS] == [v for _, v in FLAGS]
    # the other lists stay what they are, and the headers in front of this one do not name its functions
    names = set(NAMES)
    assert not names & set(rt64.exported_symbols())
    for other in (rt64.QUERY_API, rt64.SURFACE_API, rt64.MATERIAL_API):
        assert not names & set(s for _, s, _, _ in other)
    for other in ("rt64.h", "rt64_query.h", "rt64_surface.h", "rt64_material.h"):
        text = open(os.path.join(ROOT, "include", other)).read()
        assert not any(n in text for n in NAMES), other
    lib = rt64.Library()
    assert all(callable(getattr(lib, m)) for m, _ in _declared())
