/*
 * rt64_material.h -- material records for the hits of a ray query (MI355X extension of librt64.so).
 *
 * RT64_ResolveViewRayHits (rt64_surface.h) answers where a hit is and which way it faces.  What the surface looks like there -- the decoded
 * colour combiner of the instance's shader, the vertex colour inputs, the three texture slots and the sampler state, diffuseColorMix, the
 * alpha multipliers, uvDetailScale -- lives only inside the library after the scene is sent.  The functions here turn hit records into
 * material records with the device functions the frame's any-hit programs run (vertex fetch, combiner, software sampler), so a record
 * agrees with the picture.  They live in a header of their own and are resolved with their own loader, RT64_LoadLibraryMaterial, from the
 * handle RT64_LoadLibrary returned.
 *
 * Semantics (rules H1-H12):
 *   H1  record i is made from ray i, hit i and lods[i] (lods = NULL: 0 for every record), in the order given.  A miss (hit.instance < 0)
 *       and a bad hit (instance >= the frame's instance count, or primitive >= that instance's triangle count) give A2 / A3's record:
 *       every float 0, lod 0, instance -1, primitive 0xFFFFFFFF, flags 0 or RT64_MATERIAL_BAD_HIT; nothing is read through such an index.
 *   H2  barycentrics b = (1 - u - v, u, v), vertex fetch and the interpolation of UV and combiner inputs are the frame's (A4);
 *       RT64_MATERIAL_BACK_FACE is A6: dot(geometricNormal, ray.direction) > 0.
 *   H3  the clamped lod of a texture with `mips` levels is clamp(lod, 0, mips - 1); NaN and negative values give 0.  A POINT sampler reads
 *       level (int)(lod + 0.5); a LINEAR sampler blends levels floor(lod) and min(floor(lod) + 1, mips - 1) by the fraction.  One lod
 *       value serves the three textures of the hit, clamped per texture.  The record's `lod` is the diffuse texture's clamped value, or 0
 *       without RT64_MATERIAL_TEXTURED.
 *   H4  t0 is the diffuse texel at the interpolated UV under the shader's filter and addressing, its rgb lerped to diffuseColorMix.rgb by
 *       max(-diffuseColorMix.w, 0), its alpha kept.  t1 is the placeholder (1, 0, 1, 1).
 *   H5  color = the combiner result (alpha from the separate alpha formula when the shader has one), rgb lerped to diffuseColorMix.rgb by
 *       max(diffuseColorMix.w, 0), alpha = clamp(solidAlphaMultiplier * a, 0, 1).  float32, no UNORM8 rounding.
 *   H6  texture-edge shader: alpha > 0.3 becomes 1; otherwise alpha stays as computed and RT64_MATERIAL_CUTOUT is set (a frame's surface
 *       ray ignores such a hit).  The rest of the record is filled all the same.
 *   H7  noise shader: alpha is the value before the frame's per-pixel, per-frame 0 / 1 factor; RT64_MATERIAL_NOISE_ALPHA is set.
 *   H8  shadingNormal is A7's.  When the shader has normal mapping and a UV layout and the instance a normal texture, it is perturbed as
 *       the frame does it: tangent and binormal of the triangle's UVs through objectToWorldNormal, both sign-flipped on a back face, the
 *       texel c = 2 texel - 1 at uv * uvDetailScale, normal = normalize(n c.z + t c.x + b c.y).  No SNORM16 rounding.
 *       RT64_MATERIAL_NORMAL_MAPPED is set when that happened.
 *   H9  specular = (1, 1, 1), or the specular texel's rgb at uv * uvDetailScale with RT64_MATERIAL_SPECULAR_MAPPED.  Not quantised.
 *   H10 shadowAlpha is what a frame's shadow ray subtracts at this hit, before noise: the combiner's alpha with the diffuse texel taken at
 *       level 0 whatever lods says (and not mixed), times shadowAlphaMultiplier, clamped to 0 .. 1.  Texture-edge shader: a value > 0.3
 *       becomes 1, otherwise it is kept and RT64_MATERIAL_SHADOW_CUTOUT is set.
 *   H11 lifetime and refusals are Q7 / A9's, and one more: the calls read the frame's texture table and texel arrays, so they are refused
 *       (0, RT64_GetLastError set) after RT64_DestroyTexture on a texture the frame's table holds, until the next draw.  RT64_DestroyTexture
 *       first waits for queries still enqueued on caller streams.  The trace and surface calls read no texture and are not refused by
 *       this.  count = 0 succeeds and touches nothing.
 *   H12 not in the record: fog, the depthBias shift of t, flow, the material constants the host set itself, the sky.
 */
#ifndef RT64_MATERIAL_H_INCLUDED
#define RT64_MATERIAL_H_INCLUDED

#include "rt64_surface.h"

typedef struct {
    float color[4];          /* rgb + alpha, float32, not quantised */
    float shadingNormal[3];  unsigned int flags;
    float specular[3];       float shadowAlpha;
    float lod;               int instance; unsigned int primitive; unsigned int reserved;
} RT64_RAY_MATERIAL;                                                                                        /* 64 B */

#define RT64_MATERIAL_VALID           0x01
#define RT64_MATERIAL_BAD_HIT         0x02
#define RT64_MATERIAL_TEXTURED        0x04   /* the combiner reads texel 0 */
#define RT64_MATERIAL_NORMAL_MAPPED   0x08
#define RT64_MATERIAL_SPECULAR_MAPPED 0x10
#define RT64_MATERIAL_CUTOUT          0x20   /* texture-edge shader, alpha <= 0.3: a frame's surface ray ignores this hit */
#define RT64_MATERIAL_SHADOW_CUTOUT   0x40   /* the same for a frame's shadow ray */
#define RT64_MATERIAL_NOISE_ALPHA     0x80   /* noise shader: frames multiply alpha by a per-pixel, per-frame 0 / 1 */
#define RT64_MATERIAL_BACK_FACE       0x100

#define RT64_MATERIAL_API_LIST(X) \
    /* `count` rays, their hits and (optionally, else NULL) one lod per record in host memory -> `count` material records in host memory.  Returns 1 after the records are written, or 0 with RT64_GetLastError set. */ \
    X(ShadeViewRayHits, RT64_ShadeViewRayHits, int, (RT64_VIEW *view, const RT64_RAY *rays, const RT64_RAY_HIT *hits, const float *lods, RT64_RAY_MATERIAL *materials, size_t count)) \
    /* The same on device memory (rays, hits, materials 16-byte aligned, lods 4-byte aligned or NULL).  stream = NULL: on the device's stream, and the call returns after \
       completion.  Otherwise the call enqueues the kernel on `stream` (a hipStream_t) behind the view's last frame and returns at once; the frame's tables, vertex and index \
       buffers and textures are kept until it has run. */ \
    X(ShadeViewRayHitsDevice, RT64_ShadeViewRayHitsDevice, int, (RT64_VIEW *view, const void *rays, const void *hits, const void *lods, void *materials, size_t count, void *stream)) \
    /* Trace and shade in one staging round trip: rays (and lods) up once, both kernels back to back, results down once.  `hits` may be NULL; `flags` are \
       RT64_TraceViewRays' (RT64_RAY_FLAG_*). */ \
    X(TraceViewRayMaterials, RT64_TraceViewRayMaterials, int, (RT64_VIEW *view, const RT64_RAY *rays, RT64_RAY_HIT *hits, const float *lods, RT64_RAY_MATERIAL *materials, size_t count, unsigned int flags))

#define RT64_X(member, symbol, ret, args) typedef ret (*member##Ptr) args;
RT64_MATERIAL_API_LIST(RT64_X)
#undef RT64_X

typedef struct {
#define RT64_X(member, symbol, ret, args) member##Ptr member;
    RT64_MATERIAL_API_LIST(RT64_X)
#undef RT64_X
} RT64_LIBRARY_MATERIAL;

RT64_INLINE RT64_LIBRARY_MATERIAL RT64_LoadLibraryMaterial(RT64_LIBRARY lib) {
    RT64_LIBRARY_MATERIAL q;
#define RT64_X(member, symbol, ret, args) q.member = lib.handle ? (member##Ptr)(RT64_DLSYM(lib.handle, #symbol)) : 0;
    RT64_MATERIAL_API_LIST(RT64_X)
#undef RT64_X
    return q;
}

RT64_STATIC_ASSERT(sizeof(RT64_RAY_MATERIAL) == 64, "RT64_RAY_MATERIAL");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_MATERIAL, color) == 0, "RT64_RAY_MATERIAL.color");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_MATERIAL, shadingNormal) == 16, "RT64_RAY_MATERIAL.shadingNormal");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_MATERIAL, flags) == 28, "RT64_RAY_MATERIAL.flags");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_MATERIAL, specular) == 32, "RT64_RAY_MATERIAL.specular");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_MATERIAL, shadowAlpha) == 44, "RT64_RAY_MATERIAL.shadowAlpha");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_MATERIAL, lod) == 48, "RT64_RAY_MATERIAL.lod");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_MATERIAL, instance) == 52, "RT64_RAY_MATERIAL.instance");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_MATERIAL, primitive) == 56, "RT64_RAY_MATERIAL.primitive");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_MATERIAL, reserved) == 60, "RT64_RAY_MATERIAL.reserved");

#endif /* RT64_MATERIAL_H_INCLUDED */
