/*
 * rt64_surface.h -- surface records for the hits of a ray query (MI355X extension of librt64.so).
 *
 * RT64_TraceViewRays (rt64_query.h) answers t, u, v, instance, primitive.  What a host needs at the hit -- where it is, which way the
 * surface faces, the normal the picture was shaded with, the texture coordinate -- lives only inside the library after RT64_SetMesh:
 * the vertex and index arrays, the instance matrices, the inverse-transpose of the drawn frame.  The functions here turn hit records
 * into surface records with the same device functions the frame's any-hit program runs, so a record agrees with the picture.  They
 * live in a header of their own and are resolved with their own loader, RT64_LoadLibrarySurface, from the handle RT64_LoadLibrary
 * returned.
 *
 * Semantics (rules A1-A9):
 *   A1 record i is made from ray i and hit i; records are written in the order given.
 *   A2 hit.instance < 0 gives the miss record: every float 0, flags 0, instance -1, primitive 0xFFFFFFFF, t = +inf.
 *   A3 the hit array is the caller's: instance >= the frame's instance count, or primitive >= that instance's triangle count, gives the
 *      miss record with flags = RT64_SURFACE_BAD_HIT, and nothing is read through such an index.  Out-of-range u, v are not an error
 *      (finite garbage or NaN comes out; no access depends on them).
 *   A4 b = (1 - u - v, u, v) over the vertices indices[3 * primitive + k] of the mesh as the host sent it; position is the object-space
 *      point (p0 b0 + p1 b1) + p2 b2 taken through the instance's objectToWorld.
 *   A5 geometricNormal = normalize(tn * objectToWorldNormal), tn = -cross(p2 - p0, p1 - p0) in object space.  Never flipped.
 *   A6 RT64_SURFACE_BACK_FACE is set iff dot(geometricNormal, ray.direction) > 0.
 *   A7 shadingNormal is the frame's normal before normal mapping and quantisation: the interpolated vertex normal, normalised (tn itself
 *      when all three components are exactly 0), through objectToWorldNormal, normalised, times -1 on a back face.
 *   A8 uv is the interpolated vertex UV and RT64_SURFACE_HAS_UV is set when the instance's shader reads a texture (its vertex layout
 *      carries UVs); otherwise uv = 0, 0.  t, instance, primitive are the hit's; reserved = 0; RT64_SURFACE_VALID on every real hit.
 *   A9 lifetime and refusals are Q7's: refused (0, RT64_GetLastError set) before the view's first frame, after RT64_SetMesh /
 *      RT64_DestroyMesh on a mesh that frame traced, for NULL arrays, misaligned device arrays and unknown flags.  count = 0 succeeds
 *      and touches nothing.  The device's tile / interleave partition does not apply.
 */
#ifndef RT64_SURFACE_H_INCLUDED
#define RT64_SURFACE_H_INCLUDED

#include "rt64_query.h"

typedef struct {
    float position[3];        unsigned int flags;
    float geometricNormal[3]; int instance;
    float shadingNormal[3];   unsigned int primitive;
    float uv[2];              float t; unsigned int reserved;
} RT64_RAY_SURFACE;                                                                                         /* 64 B */

#define RT64_SURFACE_VALID      0x1
#define RT64_SURFACE_BACK_FACE  0x2
#define RT64_SURFACE_HAS_UV     0x4
#define RT64_SURFACE_BAD_HIT    0x8

#define RT64_SURFACE_API_LIST(X) \
    /* `count` rays and their hits in host memory -> `count` surface records in host memory.  Returns 1 after the records are written, or 0 with RT64_GetLastError set. */ \
    X(ResolveViewRayHits, RT64_ResolveViewRayHits, int, (RT64_VIEW *view, const RT64_RAY *rays, const RT64_RAY_HIT *hits, RT64_RAY_SURFACE *surfaces, size_t count)) \
    /* The same on device memory (16-byte aligned).  stream = NULL: on the device's stream, and the call returns after completion.  Otherwise the call \
       enqueues the resolve on `stream` (a hipStream_t) behind the view's last frame and returns at once; the frame's tables, BLASes, vertex and index \
       buffers are kept until the resolve has run. */ \
    X(ResolveViewRayHitsDevice, RT64_ResolveViewRayHitsDevice, int, (RT64_VIEW *view, const void *rays, const void *hits, void *surfaces, size_t count, void *stream)) \
    /* Trace and resolve in one staging round trip: rays up once, both kernels back to back, results down once.  `hits` may be NULL; `flags` are \
       RT64_TraceViewRays' (RT64_RAY_FLAG_*). */ \
    X(TraceViewRaySurfaces, RT64_TraceViewRaySurfaces, int, (RT64_VIEW *view, const RT64_RAY *rays, RT64_RAY_HIT *hits, RT64_RAY_SURFACE *surfaces, size_t count, unsigned int flags))

#define RT64_X(member, symbol, ret, args) typedef ret (*member##Ptr) args;
RT64_SURFACE_API_LIST(RT64_X)
#undef RT64_X

typedef struct {
#define RT64_X(member, symbol, ret, args) member##Ptr member;
    RT64_SURFACE_API_LIST(RT64_X)
#undef RT64_X
} RT64_LIBRARY_SURFACE;

RT64_INLINE RT64_LIBRARY_SURFACE RT64_LoadLibrarySurface(RT64_LIBRARY lib) {
    RT64_LIBRARY_SURFACE q;
#define RT64_X(member, symbol, ret, args) q.member = lib.handle ? (member##Ptr)(RT64_DLSYM(lib.handle, #symbol)) : 0;
    RT64_SURFACE_API_LIST(RT64_X)
#undef RT64_X
    return q;
}

RT64_STATIC_ASSERT(sizeof(RT64_RAY_SURFACE) == 64, "RT64_RAY_SURFACE");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_SURFACE, flags) == 12, "RT64_RAY_SURFACE.flags");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_SURFACE, geometricNormal) == 16, "RT64_RAY_SURFACE.geometricNormal");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_SURFACE, instance) == 28, "RT64_RAY_SURFACE.instance");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_SURFACE, shadingNormal) == 32, "RT64_RAY_SURFACE.shadingNormal");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_SURFACE, primitive) == 44, "RT64_RAY_SURFACE.primitive");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_SURFACE, uv) == 48, "RT64_RAY_SURFACE.uv");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_SURFACE, t) == 56, "RT64_RAY_SURFACE.t");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_SURFACE, reserved) == 60, "RT64_RAY_SURFACE.reserved");

#endif /* RT64_SURFACE_H_INCLUDED */
