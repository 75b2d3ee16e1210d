"""CPU-only checks of the boundary of the texture-footprint calls (include/rt64_footprint.h): the header compiles on its own, after rt64.h and after all six
headers, as C11 and C++17, the two records are 64 bytes with the documented offsets and flag values, and librt64.so / the Python binding carry exactly the names
of RT64_FOOTPRINT_API_LIST -- in a list of their own, not in any other *_API or exported_symbols(), and in no other header."""
import ctypes as C
import os
import re
import subprocess

import pytest

import __graft_entry__ as graft

ROOT = graft.ROOT
HEADER = os.path.join(ROOT, "include", "rt64_footprint.h")
NAMES = ["RT64_GenerateViewCameraRays", "RT64_GenerateViewCameraRaysDevice", "RT64_FootprintViewRayHits", "RT64_FootprintViewRayHitsDevice",
         "RT64_TraceViewPixelFootprints"]
DIFF_FIELDS = ("dOdx", "reserved0", "dOdy", "reserved1", "dDdx", "reserved2", "dDdy", "reserved3")
DIFF_OFFSETS = [0, 12, 16, 28, 32, 44, 48, 60]
FIELDS = ("duvdx", "duvdy", "lod", "lodNormal", "lodSpecular", "flags", "dPdx", "instance", "dPdy", "primitive")
OFFSETS = [0, 8, 16, 20, 24, 28, 32, 44, 48, 60]
FLAGS = [("VALID", 0x01), ("BAD_HIT", 0x02), ("HAS_UV", 0x04), ("TEXTURED", 0x08)]
OTHER_HEADERS = ("rt64.h", "rt64_query.h", "rt64_surface.h", "rt64_material.h", "rt64_alpha.h", "rt64_lighting.h")


@pytest.fixture(scope="module")
def built():
    lib = os.path.join(graft.PKG_DIR, "librt64.so")
    if not os.path.exists(lib):
        graft.build()
    return lib


def _declared():
    text = open(HEADER).read()
    body = re.search(r"#define RT64_FOOTPRINT_API_LIST\(X\)(.*?)\n\n", text, re.S).group(1)
    return re.findall(r"X\((\w+),\s*(RT64_\w+),", body)


PROBE = r"""
#include <stdio.h>
%s
int main(void) {
    RT64_LIBRARY lib; RT64_LIBRARY_FOOTPRINT p; RT64_LIBRARY_QUERY q;
    lib.handle = 0; p = RT64_LoadLibraryFootprint(lib); q = RT64_LoadLibraryQuery(lib);
    printf("%%d %%d %%d %%d %%d", (int)sizeof(RT64_RAY_DIFFERENTIAL), (int)sizeof(RT64_RAY_FOOTPRINT), (int)sizeof(RT64_RAY), (int)sizeof(RT64_RAY_HIT),
           (int)sizeof(RT64_LIBRARY_FOOTPRINT) / (int)sizeof(void *));
""" + "".join('    printf(" %%%%d", (int)offsetof(RT64_RAY_DIFFERENTIAL, %s));\n' % f for f in DIFF_FIELDS) \
    + "".join('    printf(" %%%%d", (int)offsetof(RT64_RAY_FOOTPRINT, %s));\n' % f for f in FIELDS) + r"""
    printf("\n%%d %%d %%d %%d %%d %%d", p.GenerateViewCameraRays == 0, p.GenerateViewCameraRaysDevice == 0, p.FootprintViewRayHits == 0, p.FootprintViewRayHitsDevice == 0,
           p.TraceViewPixelFootprints == 0, q.TraceViewRays == 0);
""" + "".join('    printf(" %%%%d", RT64_FOOTPRINT_%s);\n' % n for n, _ in FLAGS) + r"""
    printf("\n");
    return 0;
}
"""
INCLUDES = {
    "alone": '#include "rt64_footprint.h"',
    "after_rt64": '#include "rt64.h"\n#include "rt64_footprint.h"',
    "after_all": "".join('#include "%s"\n' % h for h in OTHER_HEADERS) + '#include "rt64_footprint.h"',
}


@pytest.mark.parametrize("includes", sorted(INCLUDES))
@pytest.mark.parametrize("lang", ["c", "cpp"])
def test_footprint_header_compiles_and_layouts_match(tmp_path, lang, includes):
    src = tmp_path / ("probe." + lang)
    src.write_text(PROBE % INCLUDES[includes])
    exe = tmp_path / "probe"
    cc, std = ("gcc", "-std=c11") if lang == "c" else ("g++", "-std=c++17")
    subprocess.run([cc, std, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-ldl"], check=True)
    out = subprocess.run([str(exe)], stdout=subprocess.PIPE, text=True, check=True).stdout.split("\n")
    assert [int(x) for x in out[0].split()] == [64, 64, 32, 32, 5] + DIFF_OFFSETS + OFFSETS
    assert [int(x) for x in out[1].split()] == [1] * 6 + [v for _, v in FLAGS]


def test_library_exports_the_footprint_list(built):
    h = C.CDLL(built, mode=C.RTLD_LOCAL)
    declared = _declared()
    assert [s for _, s in declared] == NAMES
    for _, name in declared:
        assert hasattr(h, name), name
    exported = subprocess.run(["nm", "-D", "--defined-only", built], stdout=subprocess.PIPE, text=True, check=True).stdout
    found = sorted(set(re.findall(r"\bRT64_\w*(?:Footprint|CameraRays)\w*", exported)))
    assert found == sorted(NAMES)                       # exactly the five: no other export with those words
    # ... and none of them carries a word the other extensions' boundary tests search the exports for
    assert not [n for n in NAMES if re.search(r"Surface|Resolve|ShadeView|RayMaterial|Alpha|Visibility|LightView|Lighting", n)]


def test_python_binding_matches_the_footprint_list():
    from sm64rt_legacy_renderer_amd import rt64
    assert [(m, s) for m, s, _, _ in rt64.FOOTPRINT_API] == _declared()
    assert C.sizeof(rt64.RAY_DIFFERENTIAL) == 64 and C.sizeof(rt64.RAY_FOOTPRINT) == 64
    assert [getattr(rt64.RAY_DIFFERENTIAL, f).offset for f in DIFF_FIELDS] == DIFF_OFFSETS
    assert [getattr(rt64.RAY_FOOTPRINT, f).offset for f in FIELDS] == OFFSETS
    assert [getattr(rt64, "FOOTPRINT_" + n) for n, _ in FLAGS] == [v for _, v in FLAGS]
    # the other lists stay what they are, and the other headers do not name these functions
    names = set(NAMES)
    assert not names & set(rt64.exported_symbols())
    for other in (rt64.API, rt64.EXT_API, rt64.QUERY_API, rt64.SURFACE_API, rt64.MATERIAL_API, rt64.ALPHA_API, rt64.LIGHTING_API):
        assert not names & set(s for _, s, _, _ in other)
    for other in OTHER_HEADERS:
        text = open(os.path.join(ROOT, "include", other)).read()
        assert not any(n in text for n in NAMES), other
    lib = rt64.Library()
    assert all(callable(getattr(lib, m)) for m, _ in _declared())
