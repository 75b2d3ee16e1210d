/*
 * rt64_sampled_lighting.h -- the direct light of a hit as a frame's pixel samples it (MI355X extension of librt64.so).
 *
 * RT64_LightViewRayHits (rt64_lighting.h) has no pixel: it lights every admitted candidate once at its centre.  A frame does something else: it draws
 * min(candidates, maxLights) of them with blue noise, samples max(diSamples, 1) points on each drawn light's disc and lets a noise shader thin its shadow
 * casters, all keyed by the pixel and the frame count.  The calls here run that loop for the hits of a query, with the pixel as an INPUT: every record
 * brings its own noise key (x, y, frame), and a call may override maxLights and diSamples.  A host averages N keys into converged soft shadows at a probe
 * point, or reproduces the direct-light image of the frame just drawn pixel by pixel, in one call either way.  They live in a header of their own and are
 * resolved with their own loader, RT64_LoadLibrarySampledLighting, from the handle RT64_LoadLibrary returned.
 *
 * Semantics (rules J1-J11; L* are the light rules of tests/light_rule.py, P* those of rt64_lighting.h, K* those of rt64_alpha.h):
 *   J1  record i is made from ray i, hit i, lods[i] (lods = NULL: 0) and key i.  Misses and bad hits are P1's: all floats 0, all counts 0, drawn 0,
 *       instance -1, primitive 0xFFFFFFFF, flags 0 or RT64_SAMPLED_LIGHTING_BAD_HIT.  Nothing is read through an out-of-range index.
 *   J2  the shaded point is P2's (unquantised) and rayDirection is ray.direction as given (P3).
 *   J3  keys: record i uses keys[i].  keys = NULL: the key is (i % width, i / width, frameCount) of the view's last drawn frame, frameCount being the value
 *       that frame's light loop used (the last sub-frame's under motion blur or primary_spp); count > width * height is then refused.  Coordinates outside
 *       the frame are legal: only x % 64, y % 64 and x + y * width (wrapping in 32 bits) are formed from them.  `reserved` is ignored.
 *   J4  parameters: sampling = NULL, or a field of -1, takes the last frame's maxLights / diSamples.  An override maxLights of 0 .. 16 and an override
 *       diSamples of 0 .. 64 are accepted (there are 64 noise slices; more samples would repeat them); anything else is refused, and so is flags != 0.
 *   J5  candidates are P4's, verbatim: the scan, the 1e-6 threshold, the stop at 16, lightsAdmitted, UNLIT for a mask of 0 (no draw, no walk), TRUNCATED.
 *   J6  draws are L3's with key.frame for the frame count: lCount = min(candidates, maxLights) draws; draw s takes r = blue_noise(x, y, frame + s).red times
 *       the remaining intensity and walks the candidate slots while r >= the running sum, stopping at the last slot; the chosen slot's intensity is then
 *       subtracted from the remaining intensity and set to 0.  invProbability = remaining / chosen intensity applies only when lCount = 1; a single
 *       candidate (with maxLights >= 1) is drawn without a random number at probability 1.  `drawn`: bit k is set when candidate slot k (the k-th admitted
 *       light in list order, not the light's index) was drawn; bit 16 + k when a later draw reached slot k again after it was zeroed -- the frame then
 *       lights that candidate a second time, and so does the record.
 *   J7  one drawn light is L4's: radius = pointRadius when diSamples > 0, else 0; S = max(diSamples, 1) samples, sample j = S .. 1 at the disc point of
 *       blue_noise(x, y, frame + j) on the basis perpX = cross(-L, (0, 1, 0)) (or (1, 0, 0) when that is 0), perpY = cross(perpX, -L); Lambert, specular
 *       and the shadow term are each averaged over the samples.  unshadowed sums (diffuseColor Lambert + specularColor spec) invProbability over the draws,
 *       direct the same terms times the averaged shadow term: both from the same numbers.
 *   J8  a sample's shadow ray is P6's window (tMin = 0.1 + shadowRayBias, tMax = distance - shadowOffset, no culling) walked by K5-K7, WITH the frame's
 *       noise: a caster whose shader has the noise option multiplies its alpha by rint(next_rand(init_rand(x + y * width, frame, 16))), 0 or 1 per key.
 *       A Q6-invalid shadow ray has shadow term 1 and no walk.
 *   J9  emitted is P7's.
 *   J10 for a pixel's camera ray (RT64_GenerateViewCameraRays), its RT64_TraceViewRaysAlpha hit at the frame's lod, keys = NULL and sampling = NULL,
 *       direct + emitted is the frame's direct light of that pixel from unquantised inputs, on any maxLights / diSamples, noise casters included.
 *   J11 lifetime, refusals and counters are P9 / P10's; RT64_TraceViewRaySampledLights takes RT64_RAY_FLAG_CULL_BACK_FACING only.  Not covered: fog, GI,
 *       reflection and refraction, temporal accumulation, the transparent-light term.
 */
#ifndef RT64_SAMPLED_LIGHTING_H_INCLUDED
#define RT64_SAMPLED_LIGHTING_H_INCLUDED

#include "rt64_lighting.h"

typedef struct { unsigned int x, y, frame, reserved; } RT64_LIGHT_SAMPLE_KEY;                        /* 16 B */
typedef struct { int maxLights, diSamples; unsigned int flags, reserved; } RT64_LIGHT_SAMPLING;      /* 16 B; -1 = the last frame's value */
typedef struct {
    float direct[3];      unsigned int flags;            /* the frame's sum over its draws, shadowed (J7) */
    float unshadowed[3];  unsigned int lightsAdmitted;   /* the same draws and samples with every shadow term 1 */
    float emitted[3];     unsigned int drawn;            /* bits 0-15: candidate slot drawn; bits 16-31: slot reached again after it was zeroed (J6) */
    int instance; unsigned int primitive; unsigned int nodesVisited, trianglesTested;   /* summed over the record's shadow walks */
} RT64_RAY_SAMPLED_LIGHTING;                                                             /* 64 B */

#define RT64_SAMPLED_LIGHTING_VALID      RT64_LIGHTING_VALID
#define RT64_SAMPLED_LIGHTING_BAD_HIT    RT64_LIGHTING_BAD_HIT
#define RT64_SAMPLED_LIGHTING_BACK_FACE  RT64_LIGHTING_BACK_FACE
#define RT64_SAMPLED_LIGHTING_UNLIT      RT64_LIGHTING_UNLIT
#define RT64_SAMPLED_LIGHTING_TRUNCATED  RT64_LIGHTING_TRUNCATED

#define RT64_LIGHT_SAMPLING_MAX_LIGHTS   16
#define RT64_LIGHT_SAMPLING_MAX_SAMPLES  64

#define RT64_SAMPLED_LIGHTING_API_LIST(X) \
    /* `count` rays, their hits, (optionally, else NULL) one lod and one key per record and (optionally) the call's sampling parameters in host memory -> `count` records in host memory (J1-J9).  Returns 1 after the records are written, or 0 with RT64_GetLastError set. */ \
    X(SampleViewRayLights, RT64_SampleViewRayLights, int, (RT64_VIEW *view, const RT64_RAY *rays, const RT64_RAY_HIT *hits, const float *lods, const RT64_LIGHT_SAMPLE_KEY *keys, const RT64_LIGHT_SAMPLING *sampling, RT64_RAY_SAMPLED_LIGHTING *records, size_t count)) \
    /* The same on device memory (rays, hits, keys, records 16-byte aligned, lods 4-byte aligned or NULL; `sampling` is host memory, read before the call returns).  stream = NULL: on the device's stream, and the call returns after completion. \
       Otherwise the call enqueues the kernel on `stream` (a hipStream_t) behind the view's last frame and returns at once; the frame's tables, vertex and index buffers \
       and textures are kept until it has run. */ \
    X(SampleViewRayLightsDevice, RT64_SampleViewRayLightsDevice, int, (RT64_VIEW *view, const void *rays, const void *hits, const void *lods, const void *keys, const RT64_LIGHT_SAMPLING *sampling, void *records, size_t count, void *stream)) \
    /* RT64_TraceViewRaysAlpha (K2: the hit a frame's surface ray shades), then the records of its hits, in one staging round trip; `hits` may be NULL. */ \
    X(TraceViewRaySampledLights, RT64_TraceViewRaySampledLights, int, (RT64_VIEW *view, const RT64_RAY *rays, RT64_RAY_HIT *hits, const float *lods, const RT64_LIGHT_SAMPLE_KEY *keys, const RT64_LIGHT_SAMPLING *sampling, RT64_RAY_SAMPLED_LIGHTING *records, size_t count, unsigned int flags))

#define RT64_X(member, symbol, ret, args) typedef ret (*member##Ptr) args;
RT64_SAMPLED_LIGHTING_API_LIST(RT64_X)
#undef RT64_X

typedef struct {
#define RT64_X(member, symbol, ret, args) member##Ptr member;
    RT64_SAMPLED_LIGHTING_API_LIST(RT64_X)
#undef RT64_X
} RT64_LIBRARY_SAMPLED_LIGHTING;

RT64_INLINE RT64_LIBRARY_SAMPLED_LIGHTING RT64_LoadLibrarySampledLighting(RT64_LIBRARY lib) {
    RT64_LIBRARY_SAMPLED_LIGHTING q;
#define RT64_X(member, symbol, ret, args) q.member = lib.handle ? (member##Ptr)(RT64_DLSYM(lib.handle, #symbol)) : 0;
    RT64_SAMPLED_LIGHTING_API_LIST(RT64_X)
#undef RT64_X
    return q;
}

RT64_STATIC_ASSERT(sizeof(RT64_LIGHT_SAMPLE_KEY) == 16, "RT64_LIGHT_SAMPLE_KEY");
RT64_STATIC_ASSERT(offsetof(RT64_LIGHT_SAMPLE_KEY, x) == 0, "RT64_LIGHT_SAMPLE_KEY.x");
RT64_STATIC_ASSERT(offsetof(RT64_LIGHT_SAMPLE_KEY, y) == 4, "RT64_LIGHT_SAMPLE_KEY.y");
RT64_STATIC_ASSERT(offsetof(RT64_LIGHT_SAMPLE_KEY, frame) == 8, "RT64_LIGHT_SAMPLE_KEY.frame");
RT64_STATIC_ASSERT(offsetof(RT64_LIGHT_SAMPLE_KEY, reserved) == 12, "RT64_LIGHT_SAMPLE_KEY.reserved");
RT64_STATIC_ASSERT(sizeof(RT64_LIGHT_SAMPLING) == 16, "RT64_LIGHT_SAMPLING");
RT64_STATIC_ASSERT(offsetof(RT64_LIGHT_SAMPLING, maxLights) == 0, "RT64_LIGHT_SAMPLING.maxLights");
RT64_STATIC_ASSERT(offsetof(RT64_LIGHT_SAMPLING, diSamples) == 4, "RT64_LIGHT_SAMPLING.diSamples");
RT64_STATIC_ASSERT(offsetof(RT64_LIGHT_SAMPLING, flags) == 8, "RT64_LIGHT_SAMPLING.flags");
RT64_STATIC_ASSERT(offsetof(RT64_LIGHT_SAMPLING, reserved) == 12, "RT64_LIGHT_SAMPLING.reserved");
RT64_STATIC_ASSERT(sizeof(RT64_RAY_SAMPLED_LIGHTING) == 64, "RT64_RAY_SAMPLED_LIGHTING");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_SAMPLED_LIGHTING, direct) == 0, "RT64_RAY_SAMPLED_LIGHTING.direct");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_SAMPLED_LIGHTING, flags) == 12, "RT64_RAY_SAMPLED_LIGHTING.flags");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_SAMPLED_LIGHTING, unshadowed) == 16, "RT64_RAY_SAMPLED_LIGHTING.unshadowed");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_SAMPLED_LIGHTING, lightsAdmitted) == 28, "RT64_RAY_SAMPLED_LIGHTING.lightsAdmitted");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_SAMPLED_LIGHTING, emitted) == 32, "RT64_RAY_SAMPLED_LIGHTING.emitted");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_SAMPLED_LIGHTING, drawn) == 44, "RT64_RAY_SAMPLED_LIGHTING.drawn");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_SAMPLED_LIGHTING, instance) == 48, "RT64_RAY_SAMPLED_LIGHTING.instance");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_SAMPLED_LIGHTING, primitive) == 52, "RT64_RAY_SAMPLED_LIGHTING.primitive");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_SAMPLED_LIGHTING, nodesVisited) == 56, "RT64_RAY_SAMPLED_LIGHTING.nodesVisited");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_SAMPLED_LIGHTING, trianglesTested) == 60, "RT64_RAY_SAMPLED_LIGHTING.trianglesTested");

#endif /* RT64_SAMPLED_LIGHTING_H_INCLUDED */
