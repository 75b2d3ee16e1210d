/*
 * rt64_bounce.h -- the frame's mirror and glass rays for the hits of a ray query, and mirror chains in one walk (MI355X extension of librt64.so).
 *
 * The calls of rt64_query.h / rt64_alpha.h say where a ray hits, those of rt64_surface.h, rt64_material.h and rt64_lighting.h what is there and how bright it is.
 * The calls here hand out the SECOND ray: the ray a frame's reflection pass and its refraction pass cast from that hit -- `reflect` of the direction as given (not
 * normalised), HLSL `refract` with refractionFactor as eta and a zero vector on total internal reflection, from the frame's own point on the ray, about the mapped
 * shading normal turned towards the ray -- with the Fresnel amount the primary resolve gives the reflection.  `reflected` and `refracted` are plain RT64_RAYs: they
 * feed every walk of the family unchanged.  RT64_TraceViewRayMirrorChains follows the reflected rays itself, up to eight segments per ray in one kernel.  They live
 * in a header of their own and are resolved with their own loader, RT64_LoadLibraryBounce, from the handle RT64_LoadLibrary returned.
 *
 * Semantics (rules R1-R12):
 *   R1  record i is made from ray i, hit i and lods[i] (lods = NULL: 0).  A miss (instance < 0) gives all floats 0, flags 0, instance -1, primitive 0xFFFFFFFF and
 *       both rays as 32 zero bytes (Q6-invalid: they miss without a walk); a hit whose instance or primitive is out of range the same with
 *       flags = RT64_BOUNCE_BAD_HIT.  Nothing is read through an out-of-range index.
 *   R2  position = ray.origin + ray.direction ((t - depthBias) + depthBias), in float32 in that order: the frame's vertexPosition -- its hit record holds the sort
 *       key t - depthBias and its resolve adds the bias back -- NOT A4's interpolated point (the deliberate difference from P2).  The bias orders hits; it moves
 *       no point.
 *   R3  the normal N is H8's (the mapped shading normal at H3's lod, sign-flipped on a back face; RT64_BOUNCE_BACK_FACE is A6), unquantised as in P2.
 *   R4  reflected, for every real hit, mirror or not: origin the R2 position, direction d - 2 (N.d) N with d = ray.direction AS GIVEN, not normalised,
 *       tMin = 0.1, tMax = 100000.
 *   R5  refracted, for every real hit: direction HLSL refract(d, N, refractionFactor): with c = N.d and k = 1 - eta^2 (1 - c^2), eta d - (eta c + sqrt k) N, or
 *       the zero direction and RT64_BOUNCE_TOTAL_INTERNAL when k < 0.  Origin, tMin and tMax as R4.
 *   R6  fresnel = rf + (1 - rf) clamp(1 + N.d, 1e-6, 1)^5 reflectionFresnelFactor with rf = reflectionFactor of the hit's own instance, on a RT64_BOUNCE_MIRROR hit
 *       (reflectionFactor > 1e-6): the primary resolve's amount.  0 when the hit is not MIRROR.  reflectionFactor / refractionFactor are the material's values.
 *   R7  chains: segment 0 is RT64_TraceViewRaysAlpha on the rays, lods and flags given; where segment s is MIRROR and s + 1 < depth, segment s + 1 is
 *       RT64_TraceViewRayBounces applied to segment s's reflected ray with lods = NULL, byte for byte, and record s carries RT64_BOUNCE_CONTINUED.  Every later
 *       segment of an ended chain holds the Q5 miss hit and the R1 miss record.  Record (s, i) is element s count + i of `hits` and `bounces`.
 *   R8  nodesVisited / trianglesTested are the segment's walk under count_traversal (RT64_TraceViewRayBounces hands on its own walk's, so that R7 holds with
 *       the option on); 0 in the resolve-only calls and when the option is off.
 *   R9  against a frame: for a pixel's camera ray (RT64_GenerateViewCameraRays) whose first K2 hit is opaque and unfogged, position is the frame's
 *       RT64_IMAGE_SHADING_POSITION, fresnel the RT64_IMAGE_REFLECTION alpha of a frame without reflection passes (up to its f16 store), reflected.direction
 *       `reflect` of the stored view direction and shading normal (up to their f16 steps).
 *   R10 refusals and lifetime are K9's, texture rule included.  count = 0 succeeds and touches nothing.  Refused: unknown flags (RT64_TraceViewRayBounces takes K3's; a chain
 *       RT64_RAY_FLAG_CULL_BACK_FACING only, applied to every segment), depth outside 1..8, all three outputs NULL, misaligned device arrays.
 *   R11 ties are K4's.
 *   R12 not covered: the frame's sorted hit list (a chain follows the closest K2 hit), the Fresnel weight of later reflection passes, fog, shine, sky and the light
 *       on the mirrored hit (RT64_LightViewRayHits on a segment's ray and hit gives that), noise, refraction chains.
 */
#ifndef RT64_BOUNCE_H_INCLUDED
#define RT64_BOUNCE_H_INCLUDED

#include "rt64_alpha.h"

typedef struct {
    float fresnel, reflectionFactor, refractionFactor; unsigned int flags;             /* R6; the material's two factors */
    int instance; unsigned int primitive; unsigned int nodesVisited, trianglesTested;  /* of the segment's walk (R8) */
} RT64_RAY_BOUNCE;                                                                     /* 32 B */

#define RT64_BOUNCE_VALID           0x01
#define RT64_BOUNCE_BAD_HIT         0x02
#define RT64_BOUNCE_BACK_FACE       0x04
#define RT64_BOUNCE_MIRROR          0x08   /* reflectionFactor > 1e-6 */
#define RT64_BOUNCE_GLASS           0x10   /* refractionFactor > 1e-6 */
#define RT64_BOUNCE_TOTAL_INTERNAL  0x20   /* refract's k < 0: refracted.direction is 0 */
#define RT64_BOUNCE_CONTINUED       0x40   /* chains only: this record's reflected ray was walked as the next segment */

#define RT64_MIRROR_CHAIN_MAX_DEPTH 8

#define RT64_BOUNCE_API_LIST(X) \
    /* `count` rays, their hits and (optionally, else NULL) one lod per record in host memory -> `count` records, reflected rays and refracted rays in host memory (R1-R6); any of the three outputs may be NULL, not all.  Returns 1 after they are written, or 0 with RT64_GetLastError set. */ \
    X(BounceViewRayHits, RT64_BounceViewRayHits, int, (RT64_VIEW *view, const RT64_RAY *rays, const RT64_RAY_HIT *hits, const float *lods, RT64_RAY_BOUNCE *bounces, RT64_RAY *reflected, RT64_RAY *refracted, size_t count)) \
    /* The same on device memory (every array 16-byte aligned, lods 4-byte aligned or NULL).  stream = NULL: on the device's stream, and the call returns after completion. \
       Otherwise the call enqueues the kernel on `stream` (a hipStream_t) behind the view's last frame and returns at once; the frame's tables, vertex and index buffers \
       and textures are kept until it has run. */ \
    X(BounceViewRayHitsDevice, RT64_BounceViewRayHitsDevice, int, (RT64_VIEW *view, const void *rays, const void *hits, const void *lods, void *bounces, void *reflected, void *refracted, size_t count, void *stream)) \
    /* RT64_TraceViewRaysAlpha (K2: the hit a frame's surface ray shades), then the records of its hits, in one staging round trip; `hits` may be NULL as well. */ \
    X(TraceViewRayBounces, RT64_TraceViewRayBounces, int, (RT64_VIEW *view, const RT64_RAY *rays, RT64_RAY_HIT *hits, const float *lods, RT64_RAY_BOUNCE *bounces, RT64_RAY *reflected, RT64_RAY *refracted, size_t count, unsigned int flags)) \
    /* Per ray up to `depth` (1..8) segments in one kernel (R7): `hits` and `bounces` hold depth * count records in host memory, segment-major. */ \
    X(TraceViewRayMirrorChains, RT64_TraceViewRayMirrorChains, int, (RT64_VIEW *view, const RT64_RAY *rays, const float *lods, unsigned int depth, RT64_RAY_HIT *hits, RT64_RAY_BOUNCE *bounces, size_t count, unsigned int flags)) \
    /* The chain call on device memory; alignment and `stream` as for RT64_BounceViewRayHitsDevice. */ \
    X(TraceViewRayMirrorChainsDevice, RT64_TraceViewRayMirrorChainsDevice, int, (RT64_VIEW *view, const void *rays, const void *lods, unsigned int depth, void *hits, void *bounces, size_t count, unsigned int flags, void *stream))

#define RT64_X(member, symbol, ret, args) typedef ret (*member##Ptr) args;
RT64_BOUNCE_API_LIST(RT64_X)
#undef RT64_X

typedef struct {
#define RT64_X(member, symbol, ret, args) member##Ptr member;
    RT64_BOUNCE_API_LIST(RT64_X)
#undef RT64_X
} RT64_LIBRARY_BOUNCE;

RT64_INLINE RT64_LIBRARY_BOUNCE RT64_LoadLibraryBounce(RT64_LIBRARY lib) {
    RT64_LIBRARY_BOUNCE q;
#define RT64_X(member, symbol, ret, args) q.member = lib.handle ? (member##Ptr)(RT64_DLSYM(lib.handle, #symbol)) : 0;
    RT64_BOUNCE_API_LIST(RT64_X)
#undef RT64_X
    return q;
}

RT64_STATIC_ASSERT(sizeof(RT64_RAY_BOUNCE) == 32, "RT64_RAY_BOUNCE");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_BOUNCE, fresnel) == 0, "RT64_RAY_BOUNCE.fresnel");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_BOUNCE, reflectionFactor) == 4, "RT64_RAY_BOUNCE.reflectionFactor");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_BOUNCE, refractionFactor) == 8, "RT64_RAY_BOUNCE.refractionFactor");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_BOUNCE, flags) == 12, "RT64_RAY_BOUNCE.flags");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_BOUNCE, instance) == 16, "RT64_RAY_BOUNCE.instance");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_BOUNCE, primitive) == 20, "RT64_RAY_BOUNCE.primitive");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_BOUNCE, nodesVisited) == 24, "RT64_RAY_BOUNCE.nodesVisited");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_BOUNCE, trianglesTested) == 28, "RT64_RAY_BOUNCE.trianglesTested");

#endif /* RT64_BOUNCE_H_INCLUDED */
