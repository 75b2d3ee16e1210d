/*
 * rt64_lighting.h -- direct-light records for the hits of a ray query (MI355X extension of librt64.so).
 *
 * RT64_TraceViewRays / RT64_TraceViewRaysAlpha say where a ray hits, RT64_ResolveViewRayHits and RT64_ShadeViewRayHits what the surface is there, and
 * RT64_TraceViewRayVisibility whether a point is lit from another.  The calls here answer the question those are asked for: how bright is that point under the
 * lights of the frame just drawn.  One call runs the frame's light loop for every hit -- admission, falloff, Lambert and specular terms, one shadow ray per
 * admitted light through any number of translucent layers, self light and the eye light -- without a pixel, hence without noise: where a frame draws maxLights of
 * the candidates at random and diSamples points on each light's disc, a query lights EVERY admitted candidate ONCE, AT ITS CENTRE.  They live in a header of
 * their own and are resolved with their own loader, RT64_LoadLibraryLighting, from the handle RT64_LoadLibrary returned.
 *
 * Semantics (rules P1-P11):
 *   P1  record i is made from ray i, hit i and lods[i] (lods = NULL: 0).  A miss (instance < 0) gives all floats 0, all counts 0, instance -1, primitive
 *       0xFFFFFFFF, flags 0; a hit whose instance or primitive is out of range the same record with flags = RT64_LIGHTING_BAD_HIT.  Nothing is read through
 *       an out-of-range index.
 *   P2  the shaded point: position is A4's, the normal H8's (the mapped shading normal at H3's lod, sign-flipped on a back face; RT64_LIGHTING_BACK_FACE is
 *       A6), specular H9's.  None is quantised: the one deliberate difference from a frame, which stores SNORM16 / f16.
 *   P3  rayDirection is ray.direction AS GIVEN, not normalised: the frame's is the unnormalised far-plane target and the specular terms scale with its
 *       length.  A caller that wants the frame's value passes the frame's direction.
 *   P4  admission: lights 0 .. lightCount - 1 of the frame's table are scanned; one is admitted when groupBits & lightGroupMaskBits is set and the frame's
 *       simple intensity estimate exceeds 1e-6; the scan stops after 16 admitted lights.  lightsAdmitted is that count; RT64_LIGHTING_TRUNCATED is set iff
 *       the scan stopped at 16 with lights left unscanned.  A mask of 0 gives RT64_LIGHTING_UNLIT, direct = unshadowed = 0 and no shadow walk.
 *   P5  one light, sampled once at its position: with d the distance and L the direction to it, falloff = pow(max(1 - d / attenuationRadius, 0),
 *       attenuationExponent), Lambert = lerp(max(N.L, 0), 1, ignoreNormalFactor) falloff, spec = specular pow(max(saturate(reflect(-L, N) . -rayDirection
 *       falloff), 0), specularExponent), term = diffuseColor Lambert + specularColor spec.  unshadowed is the sum of the terms in list order, direct the sum
 *       of term visibility in list order.
 *   P6  the shadow ray: origin the P2 position, direction L, tMin = 0.1 + shadowRayBias, tMax = d - shadowOffset, no culling, walked as
 *       RT64_TraceViewRayVisibility walks (K5-K7).  A Q6-invalid shadow ray (tMin >= tMax inside shadowOffset) has visibility 1 and no walk.  lightsBlocked
 *       counts the admitted lights whose visibility is exactly 0.  A hit exactly on a light's position is unspecified (finite or NaN).
 *   P7  emitted = selfLight + eyeLightDiffuseColor max(N . -rayDirection, 0) + eyeLightSpecularColor specular pow(max(saturate(reflect(rayDirection, N) .
 *       -rayDirection), 0), specularExponent), with the colours of the frame's view description.
 *   P8  for a pixel's camera ray with the frame's rayDirection, on a view with diSamples = 0 and maxLights >= the pixel's candidate count and a scene without
 *       a noise shader, direct + emitted is the frame's direct light of that pixel from unquantised inputs (a pixel whose random walk lights one candidate
 *       twice excepted).
 *   P9  nodesVisited / trianglesTested follow count_traversal, summed over the record's shadow walks; 0 when the option is off.
 *   P10 refusals and lifetime are K9's, texture rule included.  The lights are those of the view's last drawn frame: RT64_SetSceneLights afterwards changes
 *       nothing until the next draw.  RT64_TraceViewRayLighting takes RT64_RAY_FLAG_CULL_BACK_FACING only.  count = 0 succeeds and touches nothing.
 *   P11 not covered: disc sampling, random light selection, noise, fog, GI, reflection and refraction, the temporal accumulation of a frame's direct light.
 */
#ifndef RT64_LIGHTING_H_INCLUDED
#define RT64_LIGHTING_H_INCLUDED

#include "rt64_alpha.h"

typedef struct {
    float direct[3];      unsigned int flags;            /* sum over the admitted lights, shadowed (P5) */
    float unshadowed[3];  unsigned int lightsAdmitted;   /* the same sum with every visibility = 1 */
    float emitted[3];     unsigned int lightsBlocked;    /* selfLight + eye light (P7); admitted lights whose visibility is 0 */
    int instance; unsigned int primitive; unsigned int nodesVisited, trianglesTested;   /* summed over the record's shadow walks */
} RT64_RAY_LIGHTING;                                                                     /* 64 B */

#define RT64_LIGHTING_VALID      0x01
#define RT64_LIGHTING_BAD_HIT    0x02
#define RT64_LIGHTING_BACK_FACE  0x04
#define RT64_LIGHTING_UNLIT      0x08   /* the instance's lightGroupMaskBits is 0: direct = unshadowed = 0 */
#define RT64_LIGHTING_TRUNCATED  0x10   /* 16 lights were admitted and the scan stopped with lights left */

#define RT64_LIGHTING_API_LIST(X) \
    /* `count` rays, their hits and (optionally, else NULL) one lod per record in host memory -> `count` lighting records in host memory (P1-P9).  Returns 1 after the records are written, or 0 with RT64_GetLastError set. */ \
    X(LightViewRayHits, RT64_LightViewRayHits, int, (RT64_VIEW *view, const RT64_RAY *rays, const RT64_RAY_HIT *hits, const float *lods, RT64_RAY_LIGHTING *lighting, size_t count)) \
    /* The same on device memory (rays, hits, lighting 16-byte aligned, lods 4-byte aligned or NULL).  stream = NULL: on the device's stream, and the call returns after completion. \
       Otherwise the call enqueues the kernel on `stream` (a hipStream_t) behind the view's last frame and returns at once; the frame's tables, vertex and index buffers \
       and textures are kept until it has run. */ \
    X(LightViewRayHitsDevice, RT64_LightViewRayHitsDevice, int, (RT64_VIEW *view, const void *rays, const void *hits, const void *lods, void *lighting, size_t count, void *stream)) \
    /* RT64_TraceViewRaysAlpha (K2: the hit a frame's surface ray shades), then the records of its hits, in one staging round trip; `hits` may be NULL. */ \
    X(TraceViewRayLighting, RT64_TraceViewRayLighting, int, (RT64_VIEW *view, const RT64_RAY *rays, RT64_RAY_HIT *hits, const float *lods, RT64_RAY_LIGHTING *lighting, size_t count, unsigned int flags))

#define RT64_X(member, symbol, ret, args) typedef ret (*member##Ptr) args;
RT64_LIGHTING_API_LIST(RT64_X)
#undef RT64_X

typedef struct {
#define RT64_X(member, symbol, ret, args) member##Ptr member;
    RT64_LIGHTING_API_LIST(RT64_X)
#undef RT64_X
} RT64_LIBRARY_LIGHTING;

RT64_INLINE RT64_LIBRARY_LIGHTING RT64_LoadLibraryLighting(RT64_LIBRARY lib) {
    RT64_LIBRARY_LIGHTING q;
#define RT64_X(member, symbol, ret, args) q.member = lib.handle ? (member##Ptr)(RT64_DLSYM(lib.handle, #symbol)) : 0;
    RT64_LIGHTING_API_LIST(RT64_X)
#undef RT64_X
    return q;
}

RT64_STATIC_ASSERT(sizeof(RT64_RAY_LIGHTING) == 64, "RT64_RAY_LIGHTING");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_LIGHTING, direct) == 0, "RT64_RAY_LIGHTING.direct");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_LIGHTING, flags) == 12, "RT64_RAY_LIGHTING.flags");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_LIGHTING, unshadowed) == 16, "RT64_RAY_LIGHTING.unshadowed");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_LIGHTING, lightsAdmitted) == 28, "RT64_RAY_LIGHTING.lightsAdmitted");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_LIGHTING, emitted) == 32, "RT64_RAY_LIGHTING.emitted");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_LIGHTING, lightsBlocked) == 44, "RT64_RAY_LIGHTING.lightsBlocked");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_LIGHTING, instance) == 48, "RT64_RAY_LIGHTING.instance");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_LIGHTING, primitive) == 52, "RT64_RAY_LIGHTING.primitive");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_LIGHTING, nodesVisited) == 56, "RT64_RAY_LIGHTING.nodesVisited");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_LIGHTING, trianglesTested) == 60, "RT64_RAY_LIGHTING.trianglesTested");

#endif /* RT64_LIGHTING_H_INCLUDED */
