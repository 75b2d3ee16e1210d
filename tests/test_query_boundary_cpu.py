"""CPU-only checks of the ray-query boundary (include/rt64_query.h): the header compiles on its own and after rt64.h, the two records
are 32 bytes with the documented offsets, and librt64.so / the Python binding carry exactly the names of RT64_QUERY_API_LIST."""
import ctypes as C
import os
import re
import subprocess

import pytest

import __graft_entry__ as graft

ROOT = graft.ROOT
HEADER = os.path.join(ROOT, "include", "rt64_query.h")


@pytest.fixture(scope="module")
def built():
    lib = os.path.join(graft.PKG_DIR, "librt64.so")
    if not os.path.exists(lib):
        graft.build()
    return lib


def _declared():
    text = open(HEADER).read()
    body = re.search(r"#define RT64_QUERY_API_LIST\(X\)(.*?)\n\n", text, re.S).group(1)
    return re.findall(r"X\((\w+),\s*(RT64_\w+),", body)


PROBE = r"""
#include <stdio.h>
%s
int main(void) {
    RT64_LIBRARY lib; RT64_LIBRARY_QUERY q;
    lib.handle = 0; q = RT64_LoadLibraryQuery(lib);
    printf("%%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d\n", (int)sizeof(RT64_RAY), (int)offsetof(RT64_RAY, origin), (int)offsetof(RT64_RAY, tMin),
           (int)offsetof(RT64_RAY, direction), (int)offsetof(RT64_RAY, tMax), (int)sizeof(RT64_RAY_HIT), (int)offsetof(RT64_RAY_HIT, t),
           (int)offsetof(RT64_RAY_HIT, u), (int)offsetof(RT64_RAY_HIT, v), (int)offsetof(RT64_RAY_HIT, instance), (int)offsetof(RT64_RAY_HIT, primitive),
           (int)offsetof(RT64_RAY_HIT, nodesVisited), (int)offsetof(RT64_RAY_HIT, trianglesTested));
    printf("%%d %%d %%d\n", q.TraceViewRays == 0, RT64_RAY_FLAG_CULL_BACK_FACING, RT64_RAY_FLAG_ACCEPT_FIRST_HIT);
    return 0;
}
"""


@pytest.mark.parametrize("includes", ["alone", "after_rt64"])
@pytest.mark.parametrize("lang", ["c", "cpp"])
def test_query_header_compiles_and_layouts_match(tmp_path, lang, includes):
    inc = '#include "rt64_query.h"' if includes == "alone" else '#include "rt64.h"\n#include "rt64_query.h"'
    src = tmp_path / ("probe." + lang)
    src.write_text(PROBE % inc)
    exe = tmp_path / "probe"
    cc, std = ("gcc", "-std=c11") if lang == "c" else ("g++", "-std=c++17")
    subprocess.run([cc, std, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-ldl"], check=True)
    out = subprocess.run([str(exe)], stdout=subprocess.PIPE, text=True, check=True).stdout.split("\n")
    assert [int(x) for x in out[0].split()] == [32, 0, 12, 16, 28, 32, 0, 4, 8, 12, 16, 20, 24]
    assert [int(x) for x in out[1].split()] == [1, 1, 2]


def test_library_exports_the_query_list(built):
    h = C.CDLL(built, mode=C.RTLD_LOCAL)
    declared = _declared()
    assert [s for _, s in declared] == ["RT64_TraceViewRays", "RT64_TraceViewRaysDevice", "RT64_GetViewRaytracedInstance"]
    for _, name in declared:
        assert hasattr(h, name), name


def test_python_binding_matches_the_query_list():
    from sm64rt_legacy_renderer_amd import rt64
    assert [(m, s) for m, s, _, _ in rt64.QUERY_API] == _declared()
    assert C.sizeof(rt64.RAY) == 32 and C.sizeof(rt64.RAY_HIT) == 32
    assert rt64.RAY.tMax.offset == 28 and rt64.RAY_HIT.primitive.offset == 16 and rt64.RAY_HIT.trianglesTested.offset == 24
    assert (rt64.RAY_FLAG_CULL_BACK_FACING, rt64.RAY_FLAG_ACCEPT_FIRST_HIT) == (1, 2)
    # the rt64.h list stays what it is: the query names are not among exported_symbols()
    assert not set(s for _, s in _declared()) & set(rt64.exported_symbols())
