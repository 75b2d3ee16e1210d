/*
 * rt64_radiance.h -- the colour a ray brings back, and the sky behind it (MI355X extension of librt64.so).
 *
 * rt64_layers.h promises that the per-hit calls compose as  picture = sum of weights[l] x (what layer l shows) + transmittance x background.  The calls here hand
 * out the two terms a host could not obtain: the background (RT64_SkyViewRays for a mirror, glass or GI ray that misses, RT64_SkyViewPixels for a camera ray that
 * misses) and the composed colour itself (RT64_ComposeViewRayRadiance), the secondary-ray resolve of the view's last frame -- its mirror pass -- made deterministic
 * the way P1-P11 made the light loop deterministic.  They live in a header of their own and are resolved with their own loader, RT64_LoadLibraryRadiance, from the
 * handle RT64_LoadLibrary returned.
 *
 * (The resolve is exported as RT64_ComposeViewRayRadiance: `Resolve` in an export's name belongs to rt64_surface.h's RT64_ResolveViewRayHits, and the library's
 * boundary tests hold each word to its header.)
 *
 * Semantics (rules W1-W12):
 *   W1  RT64_SkyViewRays: a ray passes Q6 or its record is all zeros (flags 0); origin, tMin and tMax are read for nothing else.  uv = fake_envmap_uv(direction as
 *       given, the frame's skyYawOffset) (E1); alpha = the sky texel's alpha at that uv, LINEAR / WRAP at level 0 -- from the tiled copy when the frame made one,
 *       the same bits -- (E3) after the diffuse multiplier and the HSL modifier, which leave alpha alone (E4, E5); color = that texel's colour when alpha >= 1, else
 *       lerp(background at fake_envmap_uv(direction, 0), sky colour, alpha) (E6), the background being the frame's raster background image or transparent black.
 *       RT64_SKY_BACKGROUND: the frame drew one.  No sky texture: color is the background term alone, alpha 0, RT64_SKY_NO_TEXTURE; uv is still reported.
 *   W2  RT64_SkyViewPixels: pixels as RT64_GenerateViewCameraRays takes them (x, y pairs, or NULL: row-major from pixel 0, F1); a pixel outside the frame
 *       extrapolates.  screenUV = ((float)p + jitter) / size of the last frame, without the half pixel of F2 (the frame's own resolve: E2); uv = the sky plane's
 *       uv for it (E2); alpha and color as W1 with the plane sampler (never the tiled copy) and the background at screenUV (E6).  Every record is RT64_SKY_VALID.
 *   W3  RT64_ComposeViewRayRadiance walks the ray's layers as T7 walks them: record (l, i) at l * count + i, the list ends at the first record with instance < 0
 *       or at maxLayers; an instance or primitive out of range ends it with RT64_RADIANCE_BAD_HIT and nothing is read through such an index; a record behind
 *       complete coverage is not read.  A Q6-invalid ray reads no hit and gives radiance, surface, transparent, light 0, transmittance 1, litLayer -1, layers 0,
 *       flags 0.  State: rem = 1, surface = transparent = 0, lit = -1.
 *   W4  a layer's colour and alpha are the combiner's at lods[i] (lods = NULL: 0) as the frame's hit record holds them: H4 / H5, a texture-edge shader's alpha 1
 *       above 0.3 (H6; a cutout, which the walk never reports, keeps its alpha), a noise shader's value before the per-pixel factor (H7), each of the four
 *       channels rounded to UNORM8.  The alpha is T7's, bit for bit, so transmittance equals RT64_WeighViewRayLayers'.
 *   W5  w = rem a.  w < 1e-6: the layer is skipped, rem unchanged.  Otherwise, in this order:
 *       position = origin + direction ((t - depthBias) + depthBias), the frame's r.dist + depthBias restated from the record in float32;
 *       on a fog-enabled instance fog = fog_from_origin(material, position, origin) -- under RT64_RADIANCE_FLAG_FOG_FROM_CAMERA fog_from_camera(position), the
 *       primary and glass resolve's choice --, transparent += fogColor (fog.a w), w *= 1 - fog.a, RT64_RADIANCE_FOGGED;
 *       lightGroupMaskBits > 0: surface += colour w; otherwise transparent += (colour w) (ambient + selfLight), ambient = ambientBaseColor + ambientNoGIColor;
 *       lit = l, for every contributing layer, lit or not; layers++; rem *= 1 - a.  Then rem <= 1e-6: RT64_RADIANCE_COVERED, stop.
 *   W6  lit >= 0: light = ambient + (sum + selfLight of the lit layer's instance), sum = the terms of P4's admitted lights times their visibilities, in table
 *       order; the point, the admission, the term and the shadow walk are P2-P6's at the lit layer's hit with rayDirection as given (position A4, mapped normal H8,
 *       specular H9).  No eye light.  A lit layer with lightGroupMaskBits 0 admits nothing.  RT64_RADIANCE_LIT; RT64_RADIANCE_TRUNCATED when the scan stopped at 16
 *       admitted lights (P4).  Under RT64_RADIANCE_FLAG_UNSHADOWED every visibility is 1 and nothing is walked: the frame's own mirror pass.  lit < 0: light = 0.
 *   W7  radiance = surface light when lit >= 0, else surface; then radiance += (sky rem + transparent), sky = W1's colour for the ray.  float32, in that order.
 *       transmittance = rem, litLayer = lit, layers = the number of layers with a weight.
 *   W8  RT64_TraceViewRayRadiance runs RT64_TraceViewRayLayers' walk (16 deep, T5) and W3-W7 in one staging round trip; hits and layers may be NULL.  Its records
 *       equal the two-step calls' byte for byte.  The records for maxLayers = m equal those of the first m layers of 16.
 *   W9  flags: RT64_RAY_FLAG_CULL_BACK_FACING (Q4; it steers the walk of W8 only, no shadow walk), RT64_RADIANCE_FLAG_UNSHADOWED, RT64_RADIANCE_FLAG_FOG_FROM_CAMERA.
 *       Every other bit is refused.  The sky calls take no flags.
 *   W10 refusals and lifetime are K9's, texture rule included; the sky texture of the last frame counts for every call here, the surface textures for the
 *       radiance calls.  count = 0 succeeds and touches nothing.  Refused: maxLayers outside 1..16, NULL rays, hits, sky or radiance arrays, misaligned device
 *       arrays (16 bytes; lods 4, pixels 8), more pixels than the frame has with pixels = NULL, a last frame that traced no instance (it kept no sky).
 *   W11 the walk's counters stay in RT64_RAY_LAYERS; the shadow walks' counters are not carried.
 *   W12 not covered: the shine lerp and the k weight a mirror pass applies afterwards (both belong to the surface the ray left, like the Fresnel share, which is
 *       not computed here: R6 gives it); refraction (the mirror pass has no refraction cut: a glass layer is an ordinary layer here, unlike T7's `refraction`);
 *       the random choice of one light and the disc samples of a frame (the sum over admitted lights at their centres stands in, P5); the noise factor; GI;
 *       differentials inside the walk (F11); slot 16 of a FULL list.
 */
#ifndef RT64_RADIANCE_H_INCLUDED
#define RT64_RADIANCE_H_INCLUDED

#include "rt64_layers.h"

typedef struct {
    float color[3];       /* W1 / W2: what the ray or pixel sees when it misses everything */
    float alpha;          /* the sky texel's alpha */
    float uv[2];          /* where the sky texture was sampled */
    unsigned int flags, reserved;
} RT64_RAY_SKY;           /* 32 B */

#define RT64_SKY_VALID       0x1   /* the ray passed Q6 (a pixel always does) */
#define RT64_SKY_NO_TEXTURE  0x2   /* the frame had no sky texture: color is the background term alone */
#define RT64_SKY_BACKGROUND  0x4   /* the frame drew a raster background */

typedef struct {
    float radiance[3];    unsigned int flags;    /* W7 */
    float surface[3];     float transmittance;   /* the lit layers' colour before the light; the background's share */
    float transparent[3]; int litLayer;          /* fog and the unlit layers; the layer the light was taken at, or -1 */
    float light[3];       unsigned int layers;   /* W6; layers with a weight */
} RT64_RAY_RADIANCE;      /* 64 B */

#define RT64_RADIANCE_VALID      0x01   /* the ray passed Q6 */
#define RT64_RADIANCE_COVERED    0x02   /* the resolve stopped at complete coverage */
#define RT64_RADIANCE_BAD_HIT    0x04   /* the list ended at a record whose instance or primitive is out of range */
#define RT64_RADIANCE_LIT        0x08   /* a layer contributed: `light` was taken at litLayer */
#define RT64_RADIANCE_FOGGED     0x10   /* a contributing layer lies on a fog-enabled instance */
#define RT64_RADIANCE_TRUNCATED  0x20   /* the light scan stopped at 16 admitted lights (P4) */

/* call flags, next to RT64_RAY_FLAG_CULL_BACK_FACING */
#define RT64_RADIANCE_FLAG_UNSHADOWED       0x100   /* every visibility is 1, nothing is walked */
#define RT64_RADIANCE_FLAG_FOG_FROM_CAMERA  0x200   /* fog by the frame's camera depth instead of the distance from the ray's origin */

#define RT64_RADIANCE_API_LIST(X) \
    /* `count` rays in host memory -> what each sees of the last frame's sky when it misses everything (W1).  Returns 1 after the records are written, or 0 with RT64_GetLastError set. */ \
    X(SkyViewRays, RT64_SkyViewRays, int, (RT64_VIEW *view, const RT64_RAY *rays, RT64_RAY_SKY *sky, size_t count)) \
    /* The same on device memory (16-byte aligned).  stream = NULL: on the device's stream, and the call returns after completion.  Otherwise the call enqueues the kernel on \
       `stream` (a hipStream_t) behind the view's last frame and returns at once; the frame's tables and textures are kept until it has run. */ \
    X(SkyViewRaysDevice, RT64_SkyViewRaysDevice, int, (RT64_VIEW *view, const void *rays, void *sky, size_t count, void *stream)) \
    /* `count` pixels (x, y pairs, or NULL: row-major from pixel 0) in host memory -> what a camera ray through each shows when it misses everything (W2). */ \
    X(SkyViewPixels, RT64_SkyViewPixels, int, (RT64_VIEW *view, const unsigned int *pixels, RT64_RAY_SKY *sky, size_t count)) \
    /* The same on device memory (sky 16-byte aligned, pixels 8-byte aligned or NULL); `stream` as above. */ \
    X(SkyViewPixelsDevice, RT64_SkyViewPixelsDevice, int, (RT64_VIEW *view, const void *pixels, void *sky, size_t count, void *stream)) \
    /* `count` rays, their maxLayers * count hits, layer-major as RT64_TraceViewRayLayers writes them, and (optionally, else NULL) one lod per ray in host memory -> the colour each ray brings back (W3-W7). */ \
    X(ComposeViewRayRadiance, RT64_ComposeViewRayRadiance, int, (RT64_VIEW *view, const RT64_RAY *rays, const RT64_RAY_HIT *hits, const float *lods, unsigned int maxLayers, RT64_RAY_RADIANCE *radiance, size_t count, unsigned int flags)) \
    /* The same on device memory (16-byte aligned, lods 4-byte aligned or NULL); `stream` as above, and the vertex and index buffers are kept as well. */ \
    X(ComposeViewRayRadianceDevice, RT64_ComposeViewRayRadianceDevice, int, (RT64_VIEW *view, const void *rays, const void *hits, const void *lods, unsigned int maxLayers, void *radiance, size_t count, unsigned int flags, void *stream)) \
    /* The walk of RT64_TraceViewRayLayers and the resolve in one staging round trip (W8): `hits` (maxLayers * count) and `layers` are optional outputs. */ \
    X(TraceViewRayRadiance, RT64_TraceViewRayRadiance, int, (RT64_VIEW *view, const RT64_RAY *rays, const float *lods, unsigned int maxLayers, RT64_RAY_HIT *hits, RT64_RAY_LAYERS *layers, RT64_RAY_RADIANCE *radiance, size_t count, unsigned int flags))

#define RT64_X(member, symbol, ret, args) typedef ret (*member##Ptr) args;
RT64_RADIANCE_API_LIST(RT64_X)
#undef RT64_X

typedef struct {
#define RT64_X(member, symbol, ret, args) member##Ptr member;
    RT64_RADIANCE_API_LIST(RT64_X)
#undef RT64_X
} RT64_LIBRARY_RADIANCE;

RT64_INLINE RT64_LIBRARY_RADIANCE RT64_LoadLibraryRadiance(RT64_LIBRARY lib) {
    RT64_LIBRARY_RADIANCE q;
#define RT64_X(member, symbol, ret, args) q.member = lib.handle ? (member##Ptr)(RT64_DLSYM(lib.handle, #symbol)) : 0;
    RT64_RADIANCE_API_LIST(RT64_X)
#undef RT64_X
    return q;
}

RT64_STATIC_ASSERT(sizeof(RT64_RAY_SKY) == 32, "RT64_RAY_SKY");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_SKY, color) == 0, "RT64_RAY_SKY.color");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_SKY, alpha) == 12, "RT64_RAY_SKY.alpha");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_SKY, uv) == 16, "RT64_RAY_SKY.uv");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_SKY, flags) == 24, "RT64_RAY_SKY.flags");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_SKY, reserved) == 28, "RT64_RAY_SKY.reserved");
RT64_STATIC_ASSERT(sizeof(RT64_RAY_RADIANCE) == 64, "RT64_RAY_RADIANCE");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_RADIANCE, radiance) == 0, "RT64_RAY_RADIANCE.radiance");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_RADIANCE, flags) == 12, "RT64_RAY_RADIANCE.flags");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_RADIANCE, surface) == 16, "RT64_RAY_RADIANCE.surface");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_RADIANCE, transmittance) == 28, "RT64_RAY_RADIANCE.transmittance");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_RADIANCE, transparent) == 32, "RT64_RAY_RADIANCE.transparent");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_RADIANCE, litLayer) == 44, "RT64_RAY_RADIANCE.litLayer");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_RADIANCE, light) == 48, "RT64_RAY_RADIANCE.light");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_RADIANCE, layers) == 60, "RT64_RAY_RADIANCE.layers");

#endif /* RT64_RADIANCE_H_INCLUDED */
