/*
 * rt64_footprint.h -- texture footprints for the hits of a ray query (MI355X extension of librt64.so).
 *
 * RT64_TraceViewRays says where a ray hits, RT64_ResolveViewRayHits / RT64_ShadeViewRayHits what the surface is there at a lod the caller supplies.  The calls
 * here supply that lod: they hand out the camera ray a pixel of the view's last frame traced, with its ray differential, and turn (ray, differential, hit) into
 * the UV gradients and the clamped mip levels the frame's surface any-hit program uses for that hit.  With footprint.lod fed to RT64_ShadeViewRayHits a host
 * reproduces the frame's texel on mip-mapped textures.  They live in a header of their own and are resolved with their own loader, RT64_LoadLibraryFootprint,
 * from the handle RT64_LoadLibrary returned.
 *
 * Semantics (rules F1-F11):
 *   F1  pixels holds `count` pairs (x, y) of unsigned int (device form: 8-byte aligned).  pixels = NULL: pixel i is (i % width, i / width) of the frame's
 *       render size, and count > width * height is refused.  Coordinates outside the frame are legal and extrapolate; nothing is read through them.  diffs may
 *       be NULL in the two generate calls (rays only).
 *   F2  the ray is the one the frame's primary_ray makes for that pixel of the view's last drawn frame, that frame's pixelJitter included (motion-blur
 *       sub-frames, active upscaler: the last sub-frame's jitter).  Origin and direction come from the frame's viewI / projectionI; the direction is NOT
 *       normalised (P3 of rt64_lighting.h).  tMin = 0.1, tMax = 100000: the frame's RT_RAY_MIN_DISTANCE / RT_RAY_MAX_DISTANCE.
 *   F3  the differential: dOdx = dOdy = 0; dDdx, dDdy are the frame's compute_ray_diffs values from cameraU d.x + cameraV d.y + cameraW and the frame's SCREEN
 *       size (resolution[2..3]: not the render size under resolutionScale or an upscaler).  Reserved words are written 0.
 *   F4  record i is made from ray i, diffs[i] and hit i.  diffs = NULL: every differential is 0 -- what a frame's secondary rays carry: gradients 0, lods 0.  A
 *       miss (instance < 0) gives all floats 0, instance -1, primitive 0xFFFFFFFF, flags 0; a hit whose instance or primitive is out of range the same record
 *       with flags = RT64_FOOTPRINT_BAD_HIT.  Nothing is read through an out-of-range index.  The reserved words of an input differential are ignored.
 *   F5  dPdx, dPdy: with N the frame's triangle normal (the transformed, normalised geometric normal), o = dO + dD t, dP = o + direction (-dot(o, N) /
 *       dot(direction, N)); `direction` is ray i's AS GIVEN.
 *   F6  with RT64_FOOTPRINT_HAS_UV, duvdx / duvdy are the frame's ddx / ddy: barycentric differentials from the world-space corners times the UV edges, as the
 *       surface any-hit program forms them -- whether or not the combiner reads texel 0.  Without HAS_UV they are 0.
 *       They carry the frame's own sign: its pinhole vector cameraW is view-space +z, behind a right-handed camera, so cameraU points to the picture's left and
 *       duvdx of a camera ray is the mirror image of the geometric derivative; the lods take lengths and do not see it.
 *   F7  lod is the frame's clamped level of the diffuse texture: rho from the texture's own width and height, log2, !(lod > 0) -> 0, then the clamp to mips - 1;
 *       taken when RT64_FOOTPRINT_TEXTURED, else 0.  lodNormal / lodSpecular are the same with the gradients times uvDetailScale and that texture's own size,
 *       under the frame's own conditions (shader option, instance flag, texture index >= 0), else 0.  The frame's quirk is kept: without TEXTURED the frame
 *       hands zero gradients to the normal and specular fetches, so both lods are 0 even though duvdx / duvdy are not.  All three are finite and within
 *       [0, mips - 1].
 *   F8  dot(direction, N) = 0, a triangle of zero area or with a degenerate UV: gradients and dPd* are unspecified (finite, inf or NaN); the lods still obey
 *       F7's range.
 *   F9  for a camera ray of F2 / F3 and its closest hit, RT64_ShadeViewRayHits with lods[i] = footprint.lod samples the diffuse texture at the frame's level;
 *       the mapped normal and specular agree as well when those textures have the diffuse texture's size and uvDetailScale = 1.  Otherwise lodNormal /
 *       lodSpecular say what the frame used.
 *   F10 refusals and lifetime are H11's (no frame, a changed or destroyed mesh, a destroyed texture: the footprint kernel reads the texture table).  The generate
 *       calls read no mesh and no texture and are refused only without a frame -- a frame that traced no instance kept no camera and counts as none ("the view's
 *       last frame traced no instance").  Alignment as in the other device forms (pixels 8 bytes); count = 0 succeeds and
 *       touches nothing; enqueued forms keep the frame's tables as the other queries do.  RT64_TraceViewPixelFootprints takes RT64_RAY_FLAG_CULL_BACK_FACING only.
 *   F11 not covered: differentials of reflected or refracted rays (the frame carries none either), anisotropic footprints, a walk that honours alpha inside
 *       the composite call (K2 needs the lod before the hit is known: call RT64_TraceViewRaysAlpha with lods of your own).
 */
#ifndef RT64_FOOTPRINT_H_INCLUDED
#define RT64_FOOTPRINT_H_INCLUDED

#include "rt64_query.h"

typedef struct {            /* d(origin)/d(pixel x), /d(pixel y), d(normalised direction)/d(pixel x), /d(pixel y) */
    float dOdx[3]; unsigned int reserved0;
    float dOdy[3]; unsigned int reserved1;
    float dDdx[3]; unsigned int reserved2;
    float dDdy[3]; unsigned int reserved3;
} RT64_RAY_DIFFERENTIAL;    /* 64 B */

typedef struct {
    float duvdx[2], duvdy[2];                                      /* UV gradients per pixel step, before any uvDetailScale (F6) */
    float lod, lodNormal, lodSpecular; unsigned int flags;         /* clamped lods of the diffuse / normal / specular texture (F7) */
    float dPdx[3]; int instance;                                   /* the differential origin projected onto the triangle's plane (F5) */
    float dPdy[3]; unsigned int primitive;
} RT64_RAY_FOOTPRINT;       /* 64 B */

#define RT64_FOOTPRINT_VALID     0x01
#define RT64_FOOTPRINT_BAD_HIT   0x02
#define RT64_FOOTPRINT_HAS_UV    0x04   /* the shader's vertex layout has a UV: the gradients are computed */
#define RT64_FOOTPRINT_TEXTURED  0x08   /* the combiner reads texel 0: the frame computes gradients for this hit */

#define RT64_FOOTPRINT_API_LIST(X) \
    /* `count` pixels (x, y pairs, or NULL: row-major from pixel 0) in host memory -> the camera rays the view's last frame traced for them and (diffs != NULL) their differentials, in host memory (F1-F3).  Returns 1 after the arrays are written, or 0 with RT64_GetLastError set. */ \
    X(GenerateViewCameraRays, RT64_GenerateViewCameraRays, int, (RT64_VIEW *view, const unsigned int *pixels, RT64_RAY *rays, RT64_RAY_DIFFERENTIAL *diffs, size_t count)) \
    /* The same on device memory (rays, diffs 16-byte aligned, pixels 8-byte aligned or NULL).  stream = NULL: on the device's stream, and the call returns after completion. \
       Otherwise the call enqueues the kernel on `stream` (a hipStream_t) behind the view's last frame and returns at once. */ \
    X(GenerateViewCameraRaysDevice, RT64_GenerateViewCameraRaysDevice, int, (RT64_VIEW *view, const void *pixels, void *rays, void *diffs, size_t count, void *stream)) \
    /* `count` rays, their differentials (or NULL: all 0) and their hits in host memory -> `count` footprint records in host memory (F4-F8). */ \
    X(FootprintViewRayHits, RT64_FootprintViewRayHits, int, (RT64_VIEW *view, const RT64_RAY *rays, const RT64_RAY_DIFFERENTIAL *diffs, const RT64_RAY_HIT *hits, RT64_RAY_FOOTPRINT *footprints, size_t count)) \
    /* The same on device memory (every array 16-byte aligned; diffs may be NULL); `stream` as above: the frame's tables, vertex and index buffers and textures are kept until an enqueued call has run. */ \
    X(FootprintViewRayHitsDevice, RT64_FootprintViewRayHitsDevice, int, (RT64_VIEW *view, const void *rays, const void *diffs, const void *hits, void *footprints, size_t count, void *stream)) \
    /* The camera rays of `count` pixels, RT64_TraceViewRays' walk (Q2: every intersection committed), then the footprints of its hits, in one staging round trip; `rays` and `hits` may be NULL. */ \
    X(TraceViewPixelFootprints, RT64_TraceViewPixelFootprints, int, (RT64_VIEW *view, const unsigned int *pixels, RT64_RAY *rays, RT64_RAY_HIT *hits, RT64_RAY_FOOTPRINT *footprints, size_t count, unsigned int flags))

#define RT64_X(member, symbol, ret, args) typedef ret (*member##Ptr) args;
RT64_FOOTPRINT_API_LIST(RT64_X)
#undef RT64_X

typedef struct {
#define RT64_X(member, symbol, ret, args) member##Ptr member;
    RT64_FOOTPRINT_API_LIST(RT64_X)
#undef RT64_X
} RT64_LIBRARY_FOOTPRINT;

RT64_INLINE RT64_LIBRARY_FOOTPRINT RT64_LoadLibraryFootprint(RT64_LIBRARY lib) {
    RT64_LIBRARY_FOOTPRINT q;
#define RT64_X(member, symbol, ret, args) q.member = lib.handle ? (member##Ptr)(RT64_DLSYM(lib.handle, #symbol)) : 0;
    RT64_FOOTPRINT_API_LIST(RT64_X)
#undef RT64_X
    return q;
}

RT64_STATIC_ASSERT(sizeof(RT64_RAY_DIFFERENTIAL) == 64, "RT64_RAY_DIFFERENTIAL");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_DIFFERENTIAL, dOdx) == 0, "RT64_RAY_DIFFERENTIAL.dOdx");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_DIFFERENTIAL, reserved0) == 12, "RT64_RAY_DIFFERENTIAL.reserved0");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_DIFFERENTIAL, dOdy) == 16, "RT64_RAY_DIFFERENTIAL.dOdy");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_DIFFERENTIAL, reserved1) == 28, "RT64_RAY_DIFFERENTIAL.reserved1");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_DIFFERENTIAL, dDdx) == 32, "RT64_RAY_DIFFERENTIAL.dDdx");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_DIFFERENTIAL, reserved2) == 44, "RT64_RAY_DIFFERENTIAL.reserved2");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_DIFFERENTIAL, dDdy) == 48, "RT64_RAY_DIFFERENTIAL.dDdy");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_DIFFERENTIAL, reserved3) == 60, "RT64_RAY_DIFFERENTIAL.reserved3");
RT64_STATIC_ASSERT(sizeof(RT64_RAY_FOOTPRINT) == 64, "RT64_RAY_FOOTPRINT");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_FOOTPRINT, duvdx) == 0, "RT64_RAY_FOOTPRINT.duvdx");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_FOOTPRINT, duvdy) == 8, "RT64_RAY_FOOTPRINT.duvdy");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_FOOTPRINT, lod) == 16, "RT64_RAY_FOOTPRINT.lod");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_FOOTPRINT, lodNormal) == 20, "RT64_RAY_FOOTPRINT.lodNormal");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_FOOTPRINT, lodSpecular) == 24, "RT64_RAY_FOOTPRINT.lodSpecular");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_FOOTPRINT, flags) == 28, "RT64_RAY_FOOTPRINT.flags");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_FOOTPRINT, dPdx) == 32, "RT64_RAY_FOOTPRINT.dPdx");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_FOOTPRINT, instance) == 44, "RT64_RAY_FOOTPRINT.instance");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_FOOTPRINT, dPdy) == 48, "RT64_RAY_FOOTPRINT.dPdy");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_FOOTPRINT, primitive) == 60, "RT64_RAY_FOOTPRINT.primitive");

#endif /* RT64_FOOTPRINT_H_INCLUDED */
