/*
 * rt64_alpha.h -- ray queries whose walk honours alpha (MI355X extension of librt64.so).
 *
 * RT64_TraceViewRays (rt64_query.h) commits every intersection, and RT64_ShadeViewRayHits (rt64_material.h) says afterwards whether a frame's
 * ray would have ignored the hit.  The two calls here run the frame's any-hit programs inside the walk itself: a closest-hit query that looks
 * through the holes of texture-edge shaders, and a visibility query that answers "is this point lit from there" as the frame's shadow rays do,
 * through any number of translucent layers.  They live in a header of their own and are resolved with their own loader, RT64_LoadLibraryAlpha,
 * from the handle RT64_LoadLibrary returned.
 *
 * Semantics (rules K1-K10):
 *   K1  the walk is RT64_TraceViewRays' (Q1, Q5, Q6, Q7): same TLAS and BLASes, object-space traversal, tMin < t < tMax, the miss record, invalid
 *       rays, refusals.  A Q6-invalid ray gives the Q5 miss record, or visibility 1 with flags 0.  Counters follow count_traversal.
 *   K2  RT64_TraceViewRaysAlpha reports the closest intersection among those RT64_ShadeViewRayHits would not flag RT64_MATERIAL_CUTOUT for the same
 *       ray and lods[i] (lods = NULL: 0): H6's alpha at H3's level.  A cutout is ignored and does not shorten the ray.  Only instances whose
 *       shader has the texture-edge option are asked; every other intersection commits as in Q2.  A noise shader is never a cutout (H7).  No
 *       depthBias key, no k-buffer.
 *   K3  RT64_RAY_FLAG_CULL_BACK_FACING is Q4; RT64_RAY_FLAG_ACCEPT_FIRST_HIT ends the walk at the first intersection K2 accepts; any other bit is
 *       refused.  The visibility calls accept RT64_RAY_FLAG_CULL_BACK_FACING only (a frame's shadow rays do not cull: pass 0 for theirs).
 *   K4  two accepted intersections at bit-equal t may be reported either way.
 *   K5  visibility starts at 1 and visits every intersection in the window, in the walk's order: on an instance that is shadow-opaque (K6) it
 *       becomes 0 and the walk ends; otherwise a = H10's shadowAlpha at level 0; RT64_MATERIAL_SHADOW_CUTOUT: the intersection is ignored;
 *       otherwise visibility = max(visibility - a, 0), and the walk ends at 0.  In exact arithmetic: max(1 - sum a, 0).
 *   K6  shadow-opaque (rule O2) is a property of the instance, decided when the frame was drawn: its shader has no alpha option; or it has neither
 *       the noise nor the texture-edge option, its alpha formula is a single input or a product of two, and the lower bound of that formula over
 *       the mesh's vertex alphas and the diffuse texture's texel alphas, times shadowAlphaMultiplier, is >= 0.999.
 *   K7  a noise shader contributes its alpha before the frame's per-pixel 0 / 1 factor: a query has no pixel.
 *   K8  on a scene without a texture-edge shader RT64_TraceViewRaysAlpha returns t, u, v, instance, primitive byte-equal to RT64_TraceViewRays; on
 *       a scene whose instances are all shadow-opaque visibility is 0 exactly where RT64_TraceViewRays(ACCEPT_FIRST_HIT) hits, and 1 elsewhere.
 *   K9  refusals and lifetime are H11's: refused before the first frame, after RT64_SetMesh / RT64_DestroyMesh on a traced mesh and after
 *       RT64_DestroyTexture on a texture the frame's table holds; RT64_DestroyTexture waits for enqueued queries; count = 0 succeeds and touches
 *       nothing; NULL arrays (other than lods), a NULL view and misaligned device arrays are refused with RT64_GetLastError set.
 *   K10 not covered: fog, the sky, refraction or reflection continuation, depthBias, light sampling.  A caller that wants a frame's shadow ray
 *       puts shadowRayBias and the light's shadowOffset into tMin / tMax itself.
 */
#ifndef RT64_ALPHA_H_INCLUDED
#define RT64_ALPHA_H_INCLUDED

#include "rt64_material.h"

typedef struct {
    float visibility;        /* 0 .. 1: what a frame's shadow ray would return, noise aside */
    unsigned int flags;
    unsigned int nodesVisited, trianglesTested;
} RT64_RAY_VISIBILITY;                                                                                      /* 16 B */

#define RT64_VISIBILITY_VALID    0x1   /* the ray passed Q6 and was walked */
#define RT64_VISIBILITY_BLOCKED  0x2   /* visibility == 0 */

#define RT64_ALPHA_API_LIST(X) \
    /* `count` rays and (optionally, else NULL) one lod per ray in host memory -> `count` hit records in host memory (K2).  Returns 1 after the hits are written, or 0 with RT64_GetLastError set. */ \
    X(TraceViewRaysAlpha, RT64_TraceViewRaysAlpha, int, (RT64_VIEW *view, const RT64_RAY *rays, const float *lods, RT64_RAY_HIT *hits, size_t count, unsigned int flags)) \
    /* The same on device memory (rays, hits 16-byte aligned, lods 4-byte aligned or NULL).  stream = NULL: on the device's stream, and the call returns after completion. \
       Otherwise the call enqueues the kernel on `stream` (a hipStream_t) behind the view's last frame and returns at once; the frame's tables, vertex and index buffers \
       and textures are kept until it has run. */ \
    X(TraceViewRaysAlphaDevice, RT64_TraceViewRaysAlphaDevice, int, (RT64_VIEW *view, const void *rays, const void *lods, void *hits, size_t count, unsigned int flags, void *stream)) \
    /* `count` rays in host memory -> `count` visibility records in host memory (K5). */ \
    X(TraceViewRayVisibility, RT64_TraceViewRayVisibility, int, (RT64_VIEW *view, const RT64_RAY *rays, RT64_RAY_VISIBILITY *visibility, size_t count, unsigned int flags)) \
    /* The same on device memory (both arrays 16-byte aligned; a record is 16 bytes), `stream` as above. */ \
    X(TraceViewRayVisibilityDevice, RT64_TraceViewRayVisibilityDevice, int, (RT64_VIEW *view, const void *rays, void *visibility, size_t count, unsigned int flags, void *stream))

#define RT64_X(member, symbol, ret, args) typedef ret (*member##Ptr) args;
RT64_ALPHA_API_LIST(RT64_X)
#undef RT64_X

typedef struct {
#define RT64_X(member, symbol, ret, args) member##Ptr member;
    RT64_ALPHA_API_LIST(RT64_X)
#undef RT64_X
} RT64_LIBRARY_ALPHA;

RT64_INLINE RT64_LIBRARY_ALPHA RT64_LoadLibraryAlpha(RT64_LIBRARY lib) {
    RT64_LIBRARY_ALPHA q;
#define RT64_X(member, symbol, ret, args) q.member = lib.handle ? (member##Ptr)(RT64_DLSYM(lib.handle, #symbol)) : 0;
    RT64_ALPHA_API_LIST(RT64_X)
#undef RT64_X
    return q;
}

RT64_STATIC_ASSERT(sizeof(RT64_RAY_VISIBILITY) == 16, "RT64_RAY_VISIBILITY");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_VISIBILITY, visibility) == 0, "RT64_RAY_VISIBILITY.visibility");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_VISIBILITY, flags) == 4, "RT64_RAY_VISIBILITY.flags");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_VISIBILITY, nodesVisited) == 8, "RT64_RAY_VISIBILITY.nodesVisited");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_VISIBILITY, trianglesTested) == 12, "RT64_RAY_VISIBILITY.trianglesTested");

#endif /* RT64_ALPHA_H_INCLUDED */
