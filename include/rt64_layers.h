/*
 * rt64_layers.h -- a ray's sorted hit list, as a frame keeps it, and the weight each of its layers gets in the frame's resolve (MI355X extension of librt64.so).
 *
 * RT64_TraceViewRaysAlpha reports the ONE hit a frame would shade first.  A frame keeps more: per ray a list of up to 16 hits, sorted by t - depthBias, which it
 * resolves front to back until coverage is complete.  The calls here hand out that list (RT64_TraceViewRayLayers: what lies behind the water surface, which decal
 * wins at a point) and the share of the picture each entry gets (RT64_WeighViewRayLayers), so that the per-hit calls of rt64_surface.h, rt64_material.h,
 * rt64_lighting.h, rt64_footprint.h and rt64_bounce.h compose layer by layer: picture = sum of weights[l] x (what layer l shows) + transmittance x background.
 * They live in a header of their own and are resolved with their own loader, RT64_LoadLibraryLayers, from the handle RT64_LoadLibrary returned.
 *
 * Semantics (rules T1-T12):
 *   T1  the walk is K1's; the accepted intersections of a ray are K2's: a texture-edge cutout at lods[i] (lods = NULL: 0) is ignored and shortens nothing.
 *       RT64_RAY_FLAG_CULL_BACK_FACING is Q4; every other flag bit is refused.
 *   T2  the key of an intersection is t - depthBias of its instance, in float32.  The list is sorted ascending by key, with strict `<` insertion; two entries with
 *       bit-equal keys may come out either way.
 *   T3  an instance is O1-opaque as the frame decided it: its shader has neither the noise nor the texture-edge option, its alpha formula is a single input or a
 *       product of two (no alpha option: the bound is 1), and the lower bound of that formula over the mesh's vertex alphas and the diffuse texels, times
 *       solidAlphaMultiplier, is >= 0.999.  The list ends with its first entry on an O1-opaque instance, and RT64_LAYERS_ENDS_OPAQUE is set: a frame's resolve
 *       never reads past that entry, and what its walk keeps behind it depends on the order of arrival.
 *   T4  shortening is the frame's: an accepted intersection on an O1-opaque instance lowers tMax to key + maxDepthBias (the largest depthBias of the frame's
 *       instances); an intersection that lands in slot 15 commits tMax = t.  Nothing else shortens the ray.
 *   T5  with E the accepted intersection on an O1-opaque instance of smallest key (if any) and "in reach" t < key_E + maxDepthBias (no E: the whole window):
 *       (a) fewer than 16 accepted intersections in the ray's window (or fewer than 16 in reach, all on instances of one depthBias): the list is exactly those
 *           with key < key_E, sorted, then E -- whatever the walk's order;
 *       (b) 16 or more, all on instances of one depthBias: the 16 smallest keys, truncated by T3;
 *       (c) otherwise: what the frame's walk keeps in its slots 0..15 for that ray in this library's traversal order, truncated by T3.
 *       The list is always built 16 deep; maxLayers (1..16) only limits what is written.
 *   T6  layers.count = min(length, maxLayers); entries l >= count of `hits` are the Q5 miss record (every byte of `hits` is written).  A layer's own
 *       nodesVisited / trianglesTested are 0; the walk's counters are RT64_RAY_LAYERS', under count_traversal.  RT64_LAYERS_ENDS_OPAQUE and RT64_LAYERS_FULL
 *       describe the list as built (16 deep), whatever maxLayers is.  A Q6-invalid ray gives count 0, flags 0 and miss records.
 *   T7  weights: rem = 1; for each layer l in order -- the list ends at the first record with instance < 0; an instance or primitive out of range ends it too,
 *       with RT64_COVERAGE_BAD_HIT, and nothing is read through such an index -- a = H5 / H6's alpha at lods[i] rounded to UNORM8 as the frame stores it (a noise
 *       shader: the value before the per-pixel factor, H7; a texture-edge shader: 1 above 0.3, and a cutout, which the walk never reports, keeps its alpha),
 *       w = rem a.  w >= 1e-6: weights[l] = w, rem *= 1 - a, shaded++, and if the instance's refractionFactor > 1e-6: refraction = rem, rem = 0,
 *       RT64_COVERAGE_GLASS.  w < 1e-6: weights[l] = 0, rem unchanged (the frame skips such a layer).  rem <= 1e-6: RT64_COVERAGE_COVERED, stop.  Later weights
 *       are 0; transmittance = rem is the background's share.  float32, in that order.  A Q6-invalid ray: weights 0, transmittance 1, flags 0, no hit is read.
 *   T8  RT64_TraceViewRayLayers with `weights` or `coverage` runs both kernels back to back; its output equals the two-step calls' byte for byte.
 *   T9  on a scene whose instances are all O1-opaque with depthBias 0 (the sample scene), layer 0 at maxLayers = 1 equals RT64_TraceViewRaysAlpha's t, u, v,
 *       instance and primitive byte for byte; with a bias they differ by design (smallest key against smallest t).  The output for maxLayers = m is the first m
 *       layers of the output for 16.
 *   T10 against a frame, for a pixel's camera ray (RT64_GenerateViewCameraRays) on a scene with mip-less edge textures and without fog, mirror or glass: layer 0
 *       is RT64_IMAGE_PRIMARY_HIT's t, u, v (bits) and primitive; 1 - transmittance is the alpha of RT64_IMAGE_DIFFUSE up to its UNORM8 store when the list
 *       is not FULL.
 *   T11 refusals and lifetime are K9's, texture rule included.  count = 0 succeeds and touches nothing.  Refused: maxLayers outside 1..16, unknown flags, NULL
 *       rays, hits or layers, NULL weights or coverage in the Weigh calls, misaligned device arrays.
 *   T12 not covered: the frame's scratch slot 16 (a frame's resolve may read a 17th entry of a FULL list); fog and the Fresnel share that scale a weight
 *       afterwards (R6 gives the Fresnel share); the transparent-light term, the noise factor, the sky; lod from ray differentials inside the walk (F11).
 */
#ifndef RT64_LAYERS_H_INCLUDED
#define RT64_LAYERS_H_INCLUDED

#include "rt64_alpha.h"

typedef struct {
    unsigned int count, flags;                   /* T6 */
    unsigned int nodesVisited, trianglesTested;  /* of the ray's walk (count_traversal) */
} RT64_RAY_LAYERS;                               /* 16 B */

#define RT64_LAYERS_VALID        0x1   /* the ray passed Q6 and was walked */
#define RT64_LAYERS_ENDS_OPAQUE  0x2   /* the list's last entry lies on an instance the frame proved opaque (rule O1) */
#define RT64_LAYERS_FULL         0x4   /* the list is 16 long and not ENDS_OPAQUE: accepted intersections behind entry 15 are not reported */

typedef struct {
    float transmittance, refraction;             /* T7: the background's share; the share a glass layer hands to its refracted ray */
    unsigned int shaded, flags;                  /* layers with a weight */
} RT64_RAY_COVERAGE;                             /* 16 B */

#define RT64_COVERAGE_VALID    0x1
#define RT64_COVERAGE_COVERED  0x2   /* the resolve stopped at complete coverage */
#define RT64_COVERAGE_GLASS    0x4   /* a weighted layer refracts: `refraction` is its ray's share */
#define RT64_COVERAGE_BAD_HIT  0x8   /* the list ended at a record whose instance or primitive is out of range */

#define RT64_RAY_LAYERS_MAX 16

#define RT64_LAYERS_API_LIST(X) \
    /* `count` rays and (optionally, else NULL) one lod per ray in host memory -> maxLayers * count RT64_RAY_HITs, layer-major (record (l, i) at l * count + i), and `count` RT64_RAY_LAYERS in host memory (T1-T6); with `weights` (maxLayers * count floats, the same order) or `coverage` not NULL the resolve of RT64_WeighViewRayLayers as well (T8), in one staging round trip.  Returns 1 after they are written, or 0 with RT64_GetLastError set. */ \
    X(TraceViewRayLayers, RT64_TraceViewRayLayers, int, (RT64_VIEW *view, const RT64_RAY *rays, const float *lods, unsigned int maxLayers, RT64_RAY_HIT *hits, RT64_RAY_LAYERS *layers, float *weights, RT64_RAY_COVERAGE *coverage, size_t count, unsigned int flags)) \
    /* The walk alone on device memory (every array 16-byte aligned, lods 4-byte aligned or NULL).  stream = NULL: on the device's stream, and the call returns after completion. \
       Otherwise the call enqueues the kernel on `stream` (a hipStream_t) behind the view's last frame and returns at once; the frame's tables, vertex and index buffers \
       and textures are kept until it has run. */ \
    X(TraceViewRayLayersDevice, RT64_TraceViewRayLayersDevice, int, (RT64_VIEW *view, const void *rays, const void *lods, unsigned int maxLayers, void *hits, void *layers, size_t count, unsigned int flags, void *stream)) \
    /* The resolve alone (T7): `count` rays, their maxLayers * count hits and (optionally) lods in host memory -> maxLayers * count weights and `count` RT64_RAY_COVERAGEs in host memory. */ \
    X(WeighViewRayLayers, RT64_WeighViewRayLayers, int, (RT64_VIEW *view, const RT64_RAY *rays, const RT64_RAY_HIT *hits, const float *lods, unsigned int maxLayers, float *weights, RT64_RAY_COVERAGE *coverage, size_t count)) \
    /* The resolve on device memory (weights 4-byte aligned); alignment and `stream` as for RT64_TraceViewRayLayersDevice. */ \
    X(WeighViewRayLayersDevice, RT64_WeighViewRayLayersDevice, int, (RT64_VIEW *view, const void *rays, const void *hits, const void *lods, unsigned int maxLayers, void *weights, void *coverage, size_t count, void *stream))

#define RT64_X(member, symbol, ret, args) typedef ret (*member##Ptr) args;
RT64_LAYERS_API_LIST(RT64_X)
#undef RT64_X

typedef struct {
#define RT64_X(member, symbol, ret, args) member##Ptr member;
    RT64_LAYERS_API_LIST(RT64_X)
#undef RT64_X
} RT64_LIBRARY_LAYERS;

RT64_INLINE RT64_LIBRARY_LAYERS RT64_LoadLibraryLayers(RT64_LIBRARY lib) {
    RT64_LIBRARY_LAYERS q;
#define RT64_X(member, symbol, ret, args) q.member = lib.handle ? (member##Ptr)(RT64_DLSYM(lib.handle, #symbol)) : 0;
    RT64_LAYERS_API_LIST(RT64_X)
#undef RT64_X
    return q;
}

RT64_STATIC_ASSERT(sizeof(RT64_RAY_LAYERS) == 16, "RT64_RAY_LAYERS");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_LAYERS, count) == 0, "RT64_RAY_LAYERS.count");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_LAYERS, flags) == 4, "RT64_RAY_LAYERS.flags");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_LAYERS, nodesVisited) == 8, "RT64_RAY_LAYERS.nodesVisited");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_LAYERS, trianglesTested) == 12, "RT64_RAY_LAYERS.trianglesTested");
RT64_STATIC_ASSERT(sizeof(RT64_RAY_COVERAGE) == 16, "RT64_RAY_COVERAGE");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_COVERAGE, transmittance) == 0, "RT64_RAY_COVERAGE.transmittance");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_COVERAGE, refraction) == 4, "RT64_RAY_COVERAGE.refraction");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_COVERAGE, shaded) == 8, "RT64_RAY_COVERAGE.shaded");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_COVERAGE, flags) == 12, "RT64_RAY_COVERAGE.flags");

#endif /* RT64_LAYERS_H_INCLUDED */
