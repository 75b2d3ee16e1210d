/*
 * rt64_indirect.h -- the indirect light of a point as a frame's pixel samples it (MI355X extension of librt64.so).
 *
 * A frame's GI pass starts at the stored position and normal of a pixel: it sends giSamples cosine-weighted bounce rays whose directions come from blue noise keyed
 * by the pixel and the frame count, resolves each ray's sorted hit list front to back through its translucent layers, draws ONE light at the surface the resolve
 * ends on, adds the sky behind what the layers leave open, and averages the samples.  The calls here run that pass for the points of a query, with the pixel as an
 * INPUT: every point brings its own noise key (x, y, frame), and a call may override giSamples, giBounces and diSamples.  A light-probe or lightmap baker averages
 * N keys at a probe point; a host that wants to reproduce or debug the frame's RT64_IMAGE_INDIRECT_LIGHT_RAW feeds the stored RT64_IMAGE_SHADING_POSITION and
 * RT64_IMAGE_SHADING_NORMAL of its pixels back in.  The pass is available whole (RT64_TraceViewPointsIndirect, RT64_TraceViewRayIndirect) and as its links:
 * the bounce rays are plain RT64_RAYs that every walk of the family takes, and RT64_ComposeViewGIRays is the shading of one ray from the layer list
 * RT64_TraceViewRayLayers wrote for it.  The calls live in a header of their own and are resolved with their own loader, RT64_LoadLibraryIndirect, from the handle
 * RT64_LoadLibrary returned.
 *
 * Semantics (rules Y1-Y12; I* are the rules of the frame's GI pass (tests/gi_rule.py), J* those of rt64_sampled_lighting.h, T* of rt64_layers.h,
 * P* of rt64_lighting.h, K* of rt64_alpha.h):
 *   Y1  points.  A point is a position, a normal and an instance.  The normal is used as given, NOT normalised, as the frame uses the f16 normal it stored.  `instance`
 *       is informational: it is echoed in the record, -1 is allowed and it gates nothing -- an explicit point always counts as a surface.  A point whose position or
 *       normal is not finite, or whose normal is (0, 0, 0), is answered with a zeroed record flagged RT64_INDIRECT_BAD_POINT (its instance still echoed) and is never
 *       walked.  A point with RT64_GI_POINT_NONE in `flags` stands for "no point here" (the miss of RT64_TraceViewRayIndirect): all floats 0, all counts 0, flags 0,
 *       instance -1.  Other bits of `flags` are ignored.
 *   Y2  keys are RT64_LIGHT_SAMPLE_KEYs with J3's semantics: record i uses keys[i]; keys = NULL: the key is (i % width, i / width, frameCount) of the view's last
 *       drawn frame, and count > width * height is refused.  Coordinates outside the frame are legal.
 *   Y3  parameters: sampling = NULL, or a field of -1, takes the last frame's giSamples and diSamples and the device option gi_bounces.  giSamples 0 .. 64,
 *       giBounces 1 .. 2 and diSamples 0 .. 64 are accepted, anything else is refused, and so is flags != 0.  RT64_GenerateViewPointGIRays needs giSamples >= 1.
 *   Y4  the bounce ray of sample `slot` (slot = giSamples .. 1, the order the frame takes them in): origin = the point, direction = the frame's
 *       cosine-weighted direction about the normal from blue-noise slice key.frame + slot * (64 / giSamples) at (key.x, key.y) (I2, I3), NOT normalised,
 *       tMin = 0.1, tMax = 100000.  With RT64_GI_RAYS_SECOND_BOUNCE the slice is the second bounce's (I9): + (m > 1 ? m / 2 : 1), m = 64 / giSamples.  A bad point
 *       or RT64_GI_POINT_NONE gives the ray (0, 0, 0; 0; 0, 0, 0; 0), which every walk answers with a miss (Q6).  slot < 1 or slot > giSamples is refused.
 *   Y5  the resolve of one ray (I5), from records (l, i) at l * count + i as RT64_TraceViewRayLayers wrote them for the ray with
 *       RT64_RAY_FLAG_CULL_BACK_FACING and lods = NULL: layer by layer, colour = the frame's hit colour at level 0 (UNORM8, the noise option of a shader keyed by the
 *       key as K7's); a layer contributes when remaining * alpha >= 1e-6: radiance-to-be += rgb * that product, remaining *= 1 - alpha; the loop ends when
 *       remaining <= 1e-6, at the list's end (instance < 0) or at a record whose instance or primitive is out of range (RT64_GI_SAMPLE_BAD_HIT; nothing is read
 *       through it).  There is no fog and no lit / unlit split.  position = origin + direction * ((t - depthBias) + depthBias), normal (the mapped shading
 *       normal at level 0, flipped on a back face, SNORM16 as the frame's hit list stores it), specular (material specularColor times the UNORM8 specular texel)
 *       and instance are those of the LAST contributing layer (RT64_GI_SAMPLE_SURFACE; `layers` counts the contributing ones).  Where the resolve ends on no
 *       surface, position and normal are 0 and instance is -1.  A Q6-invalid ray reads no record: all floats 0, all counts 0, flags 0, instance -1.
 *   Y6  the light at that point: J5's candidates, ONE draw (J6 with maxLights = 1: the single-draw weight remaining intensity / chosen intensity; the random number is
 *       slice key.frame + 0 -- the same for every sample and bounce of a key), J7's disc samples by diSamples, J8's shadow walk with noise casters, the view vector
 *       being the ray's direction; plus the instance's selfLight.  A light group mask of 0 draws nothing (RT64_GI_SAMPLE_UNLIT).
 *   Y7  radiance = ambientBase + ((rgb * (1 - remaining)) * (incoming + light)) * giDiffuseStrength   [only with RT64_GI_SAMPLE_SURFACE]
 *                  + sky(direction) * (giSkyStrength * remaining)                                      (I7, I8; the sky is RT64_SkyViewRays' colour)
 *       `incoming` (3 floats per ray) stands where the frame's second bounce stands; NULL: ambientBase + ambientNoGI.
 *   Y8  RT64_TraceViewPointsIndirect is the chain, per sample s = giSamples .. 1: Y4's ray -> RT64_TraceViewRayLayers (16 layers, RT64_RAY_FLAG_CULL_BACK_FACING,
 *       lods NULL) -> for giBounces = 2: Y4's second-bounce ray from the resolved position and normal -> walk -> Y5-Y7 with incoming = NULL, whose radiance is the
 *       first ray's `incoming` -> Y5-Y7.  Then I10: indirect = lerp(indirect, radiance, rcp(h)), h = 1 .. giSamples, with the frame's approximate reciprocal; and
 *       I11: moments = (sum of L, sum of L^2) / giSamples, L = 0.2126 r + 0.7152 g + 0.0722 b of each sample's radiance.  `samples` is the history length as a float
 *       (= giSamples).  giSamples = 0 is I1: indirect = ambientBase + ambientNoGI, samples 0, moments 0, no ray.  There is no history: every call starts from nothing.
 *       The optional `samples` output holds the first bounce's RT64_GI_SAMPLE of sample slot s of point i at (giSamples - s) * count + i.
 *       `rays` counts the valid rays walked for the point, second bounces included; the counters sum their bounce walks and shadow walks.
 *   Y9  for the stored RT64_IMAGE_SHADING_POSITION / RT64_IMAGE_SHADING_NORMAL of a pixel with RT64_IMAGE_INSTANCE_ID >= 0, keys = NULL and sampling = NULL,
 *       `indirect`, `samples` and `moments` are what the frame's GI pass computes for that pixel before it rounds to f16 and without history (I1-I12).
 *   Y10 RT64_TraceViewRayIndirect: RT64_TraceViewRaysAlpha (K2), then the point of each hit -- position P2, the mapped shading normal at lods[i], flipped on a back
 *       face, the hit's instance -- then Y8, in one staging round trip per chunk.  A miss or a bad hit is RT64_GI_POINT_NONE (P1's convention: zero record,
 *       instance -1).  `flags`: RT64_RAY_FLAG_CULL_BACK_FACING only.
 *   Y11 lifetime and refusals are P9 / P10's: every call reads the tables of the view's last drawn frame; a refusal returns 0 with RT64_GetLastError set to a message
 *       that starts with the function's name and a colon; count = 0 succeeds and touches nothing.  The device forms take 16-byte aligned arrays (incoming: 4-byte);
 *       stream = NULL runs on the device's stream and returns after completion, otherwise the whole chain is enqueued on `stream` behind the view's last frame.
 *       The chain's scratch (rays, layer lists, samples) is the library's, giSamples * 16 hit records per point of a chunk of at most
 *       max(1, 2^20 / (16 giSamples)) points -- at most 32 MB of hit records per bounce whatever `count` is; longer calls run chunk after chunk.
 *   Y12 counters (nodesVisited, trianglesTested) are 0 unless the device option count_traversal is set; no other field depends on it.  Not covered: history and
 *       temporal accumulation, the denoiser, primary_spp, differentials of the bounce ray (level 0, as the frame), fog.
 */
#ifndef RT64_INDIRECT_H_INCLUDED
#define RT64_INDIRECT_H_INCLUDED

#include "rt64_sampled_lighting.h"
#include "rt64_layers.h"

typedef struct { float position[3]; unsigned int flags; float normal[3]; int instance; } RT64_GI_POINT;              /* 32 B */
typedef struct { int giSamples, giBounces, diSamples; unsigned int flags; } RT64_GI_SAMPLING;                        /* 16 B; -1 = the last frame's value */
typedef struct {
    float radiance[3];  float remaining;           /* Y7; the coverage the layers leave for the sky */
    float position[3];  unsigned int flags;        /* of the last contributing layer (Y5) */
    float normal[3];    int instance;
    unsigned int layers, reserved;                 /* contributing layers */
    unsigned int nodesVisited, trianglesTested;    /* of the shadow walks */
} RT64_GI_SAMPLE;                                  /* 64 B */
typedef struct {
    float indirect[3];  float samples;             /* Y8; the history length, = giSamples */
    float moments[2];   unsigned int flags; int instance;
    unsigned int rays, nodesVisited, trianglesTested, reserved;
} RT64_POINT_INDIRECT;                             /* 48 B */

#define RT64_GI_POINT_NONE           0x1u          /* in RT64_GI_POINT.flags: no point (Y1) */
#define RT64_GI_RAYS_SECOND_BOUNCE   0x1u          /* `flags` of RT64_GenerateViewPointGIRays: the second bounce's slice (Y4) */

#define RT64_GI_SAMPLE_VALID      0x01u            /* the ray passed Q6 */
#define RT64_GI_SAMPLE_BAD_HIT    0x02u
#define RT64_GI_SAMPLE_SURFACE    0x04u            /* the resolve ended on a surface: position, normal, instance hold it */
#define RT64_GI_SAMPLE_COVERED    0x08u            /* remaining <= 1e-6 */
#define RT64_GI_SAMPLE_UNLIT      0x10u
#define RT64_GI_SAMPLE_TRUNCATED  0x20u            /* J5: more than 16 candidates */

#define RT64_INDIRECT_VALID       0x01u
#define RT64_INDIRECT_BAD_POINT   0x02u
#define RT64_INDIRECT_BAD_HIT     0x04u            /* one of the point's samples has RT64_GI_SAMPLE_BAD_HIT */

#define RT64_GI_SAMPLING_MAX_SAMPLES  64
#define RT64_GI_SAMPLING_MAX_BOUNCES  2

#define RT64_INDIRECT_API_LIST(X) \
    /* `count` points, (optionally, else NULL) one key per point and the call's sampling parameters in host memory -> the bounce ray of sample `slot` of every point (Y4).  Returns 1 after the rays are written, or 0 with RT64_GetLastError set. */ \
    X(GenerateViewPointGIRays, RT64_GenerateViewPointGIRays, int, (RT64_VIEW *view, const RT64_GI_POINT *points, const RT64_LIGHT_SAMPLE_KEY *keys, const RT64_GI_SAMPLING *sampling, unsigned int slot, unsigned int flags, RT64_RAY *rays, size_t count)) \
    /* The same on device memory (16-byte aligned; `sampling` is host memory, read before the call returns); stream as Y11 has it. */ \
    X(GenerateViewPointGIRaysDevice, RT64_GenerateViewPointGIRaysDevice, int, (RT64_VIEW *view, const void *points, const void *keys, const RT64_GI_SAMPLING *sampling, unsigned int slot, unsigned int flags, void *rays, size_t count, void *stream)) \
    /* `count` rays, their maxLayers * count layer records (layer-major), optional keys, optional `incoming` (3 floats per ray) -> `count` RT64_GI_SAMPLEs (Y5-Y7). */ \
    X(ComposeViewGIRays, RT64_ComposeViewGIRays, int, (RT64_VIEW *view, const RT64_RAY *rays, const RT64_RAY_HIT *layerHits, unsigned int maxLayers, const RT64_LIGHT_SAMPLE_KEY *keys, const float *incoming, const RT64_GI_SAMPLING *sampling, RT64_GI_SAMPLE *samples, size_t count)) \
    X(ComposeViewGIRaysDevice, RT64_ComposeViewGIRaysDevice, int, (RT64_VIEW *view, const void *rays, const void *layerHits, unsigned int maxLayers, const void *keys, const void *incoming, const RT64_GI_SAMPLING *sampling, void *samples, size_t count, void *stream)) \
    /* The chain (Y8): `count` points -> `count` RT64_POINT_INDIRECTs and (samples != NULL) giSamples * count RT64_GI_SAMPLEs, sample-major. */ \
    X(TraceViewPointsIndirect, RT64_TraceViewPointsIndirect, int, (RT64_VIEW *view, const RT64_GI_POINT *points, const RT64_LIGHT_SAMPLE_KEY *keys, const RT64_GI_SAMPLING *sampling, RT64_GI_SAMPLE *samples, RT64_POINT_INDIRECT *records, size_t count)) \
    X(TraceViewPointsIndirectDevice, RT64_TraceViewPointsIndirectDevice, int, (RT64_VIEW *view, const void *points, const void *keys, const RT64_GI_SAMPLING *sampling, void *samples, void *records, size_t count, void *stream)) \
    /* RT64_TraceViewRaysAlpha, the points of its hits, then the chain (Y10); `hits` may be NULL. */ \
    X(TraceViewRayIndirect, RT64_TraceViewRayIndirect, int, (RT64_VIEW *view, const RT64_RAY *rays, RT64_RAY_HIT *hits, const float *lods, const RT64_LIGHT_SAMPLE_KEY *keys, const RT64_GI_SAMPLING *sampling, RT64_POINT_INDIRECT *records, size_t count, unsigned int flags))

#define RT64_X(member, symbol, ret, args) typedef ret (*member##Ptr) args;
RT64_INDIRECT_API_LIST(RT64_X)
#undef RT64_X

typedef struct {
#define RT64_X(member, symbol, ret, args) member##Ptr member;
    RT64_INDIRECT_API_LIST(RT64_X)
#undef RT64_X
} RT64_LIBRARY_INDIRECT;

RT64_INLINE RT64_LIBRARY_INDIRECT RT64_LoadLibraryIndirect(RT64_LIBRARY lib) {
    RT64_LIBRARY_INDIRECT q;
#define RT64_X(member, symbol, ret, args) q.member = lib.handle ? (member##Ptr)(RT64_DLSYM(lib.handle, #symbol)) : 0;
    RT64_INDIRECT_API_LIST(RT64_X)
#undef RT64_X
    return q;
}

RT64_STATIC_ASSERT(sizeof(RT64_GI_POINT) == 32, "RT64_GI_POINT");
RT64_STATIC_ASSERT(offsetof(RT64_GI_POINT, position) == 0, "RT64_GI_POINT.position");
RT64_STATIC_ASSERT(offsetof(RT64_GI_POINT, flags) == 12, "RT64_GI_POINT.flags");
RT64_STATIC_ASSERT(offsetof(RT64_GI_POINT, normal) == 16, "RT64_GI_POINT.normal");
RT64_STATIC_ASSERT(offsetof(RT64_GI_POINT, instance) == 28, "RT64_GI_POINT.instance");
RT64_STATIC_ASSERT(sizeof(RT64_GI_SAMPLING) == 16, "RT64_GI_SAMPLING");
RT64_STATIC_ASSERT(offsetof(RT64_GI_SAMPLING, giSamples) == 0, "RT64_GI_SAMPLING.giSamples");
RT64_STATIC_ASSERT(offsetof(RT64_GI_SAMPLING, giBounces) == 4, "RT64_GI_SAMPLING.giBounces");
RT64_STATIC_ASSERT(offsetof(RT64_GI_SAMPLING, diSamples) == 8, "RT64_GI_SAMPLING.diSamples");
RT64_STATIC_ASSERT(offsetof(RT64_GI_SAMPLING, flags) == 12, "RT64_GI_SAMPLING.flags");
RT64_STATIC_ASSERT(sizeof(RT64_GI_SAMPLE) == 64, "RT64_GI_SAMPLE");
RT64_STATIC_ASSERT(offsetof(RT64_GI_SAMPLE, radiance) == 0, "RT64_GI_SAMPLE.radiance");
RT64_STATIC_ASSERT(offsetof(RT64_GI_SAMPLE, remaining) == 12, "RT64_GI_SAMPLE.remaining");
RT64_STATIC_ASSERT(offsetof(RT64_GI_SAMPLE, position) == 16, "RT64_GI_SAMPLE.position");
RT64_STATIC_ASSERT(offsetof(RT64_GI_SAMPLE, flags) == 28, "RT64_GI_SAMPLE.flags");
RT64_STATIC_ASSERT(offsetof(RT64_GI_SAMPLE, normal) == 32, "RT64_GI_SAMPLE.normal");
RT64_STATIC_ASSERT(offsetof(RT64_GI_SAMPLE, instance) == 44, "RT64_GI_SAMPLE.instance");
RT64_STATIC_ASSERT(offsetof(RT64_GI_SAMPLE, layers) == 48, "RT64_GI_SAMPLE.layers");
RT64_STATIC_ASSERT(offsetof(RT64_GI_SAMPLE, reserved) == 52, "RT64_GI_SAMPLE.reserved");
RT64_STATIC_ASSERT(offsetof(RT64_GI_SAMPLE, nodesVisited) == 56, "RT64_GI_SAMPLE.nodesVisited");
RT64_STATIC_ASSERT(offsetof(RT64_GI_SAMPLE, trianglesTested) == 60, "RT64_GI_SAMPLE.trianglesTested");
RT64_STATIC_ASSERT(sizeof(RT64_POINT_INDIRECT) == 48, "RT64_POINT_INDIRECT");
RT64_STATIC_ASSERT(offsetof(RT64_POINT_INDIRECT, indirect) == 0, "RT64_POINT_INDIRECT.indirect");
RT64_STATIC_ASSERT(offsetof(RT64_POINT_INDIRECT, samples) == 12, "RT64_POINT_INDIRECT.samples");
RT64_STATIC_ASSERT(offsetof(RT64_POINT_INDIRECT, moments) == 16, "RT64_POINT_INDIRECT.moments");
RT64_STATIC_ASSERT(offsetof(RT64_POINT_INDIRECT, flags) == 24, "RT64_POINT_INDIRECT.flags");
RT64_STATIC_ASSERT(offsetof(RT64_POINT_INDIRECT, instance) == 28, "RT64_POINT_INDIRECT.instance");
RT64_STATIC_ASSERT(offsetof(RT64_POINT_INDIRECT, rays) == 32, "RT64_POINT_INDIRECT.rays");
RT64_STATIC_ASSERT(offsetof(RT64_POINT_INDIRECT, nodesVisited) == 36, "RT64_POINT_INDIRECT.nodesVisited");
RT64_STATIC_ASSERT(offsetof(RT64_POINT_INDIRECT, trianglesTested) == 40, "RT64_POINT_INDIRECT.trianglesTested");
RT64_STATIC_ASSERT(offsetof(RT64_POINT_INDIRECT, reserved) == 44, "RT64_POINT_INDIRECT.reserved");

#endif /* RT64_INDIRECT_H_INCLUDED */
