// lighting.hip -- direct-light records for the hits of a ray query (RT64_LightViewRayHits, include/rt64_lighting.h; rules P1-P11 in DESIGN.md 4).
//
// A resolve kernel of query_common.h that also walks: per record it reads 64 bytes (ray + hit, 16-byte loads) and one optional float (the lod), rebuilds the shaded
// point as hit_surface_kernel and hit_material_kernel do (position, mapped normal, specular texel: P2), then runs the frame's light loop without a pixel: every
// admitted light once, at its centre, each behind visibility_query_kernel's shadow walk (P4-P6).  It writes 64 bytes (four 16-byte stores).
//   fill_cache / lane_stack / use_cache and the spill slab are the walk kernels'; load_ray / load_hit the resolve kernels'.
//   The hit's own instance is read by material.hip's scheme: scalar loads for a wave whose hits agree on it, per-lane inst_view otherwise.  Only the fields P2-P7
//   read are used (no combiner colour); the compiler drops the rest of inst_view's loads.
//   The light loop is uniform in `l`: P.lights + l is a scalar load, admission and the term are per lane, and a lane walks only for a light it admitted.  Nothing is
//   drawn, so the candidate columns of compute_lights_random (shade.h:646-656) are not needed.
//   The shaded point, the eye light, the light sample and the shadow walk are query_shading.h's (point_of_hit, eye_light, light_sample, sample_visibility): one copy
//   for this kernel, hit_sampled_light_kernel and ray_radiance_kernel; the walk is visibility_query_kernel's own (shadow_visibility has the open defect of its
//   `waterfall` handler).  What is this file's is the miss record, the admission loop and the record.
// The arithmetic is shade.h's: light_intensity_simple (:581-589) is called; one light is compute_light (:592-633) with radius 0 and one sample (samplePosition = the
// light's position, rs = 1), the visibility kept apart from the term so that `unshadowed` and `direct` come from the same numbers.
#include "query_shading.h"

namespace {

template <bool CACHED>
__global__ __launch_bounds__(RT_BLOCK) void hit_light_kernel(FrameParams Pv, const RT64_RAY *rays, const RT64_RAY_HIT *hits, const float *lods, RT64_RAY_LIGHTING *lighting, uint64_t count) {
    PRef P = *kernel_params(); (void)Pv;
    __shared__ uint32_t ldsStack[QUERY_STACK_WORDS(CACHED) * RT_BLOCK];
    extern __shared__ u32x4_lds dynLds[];
    fill_cache<CACHED>(P, dynLds);
    TraceStack stk = lane_stack<CACHED>(P, ldsStack);
    if (CACHED) stk.use_cache(dynLds);
    const uint64_t stride = query_stride();
    for (uint64_t i = query_first(); i < count; i += stride) {
        const QueryRay ray = load_ray(QUERY_IN(rays + i));          // (a record does not depend on the origin: that load is dead code)
        const QueryHit h = load_hit(QUERY_IN(hits + i));
        const float lod = lods ? load_global(lods + i) : 0.0f;
        const f3 rayDirection = mk3(ray.d[0], ray.d[1], ray.d[2]);          // P3: as given
        const uint32_t instance = h.instance, prim = h.prim;
        const float u = h.u, v = h.v;
        // P1: the miss record; nothing below reads through an index that is out of range
        LightPoint pt;
        pt.position = pt.normal = pt.specular = pt.selfLight = mk3s(0.0f); pt.ignoreNormalFactor = pt.shadowRayBias = pt.specularExponent = 0.0f; pt.mask = 0u;
        pt.flags = (int32_t)instance < 0 ? 0u : (uint32_t)RT64_LIGHTING_BAD_HIT;
        bool real = false;
        if (instance < P.instanceCount) {               // (unsigned: a negative instance is past the end)
            const uint32_t k0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)instance);
            if (__ballot(instance != k0) == 0ull) {     // the lanes in here agree: k0 is wave-uniform, inst_view's loads are scalar and the map branches uniform
                if (prim < load_const(&P.instances[k0].triCount)) { point_of_hit(P, inst_view(P, k0), prim, u, v, rayDirection, lod, pt); real = true; }
            }
            else if (prim < load_const(&P.instances[instance].triCount)) { point_of_hit(P, inst_view(P, instance), prim, u, v, rayDirection, lod, pt); real = true; }
        }
        f3 direct = mk3s(0.0f), unshadowed = mk3s(0.0f), emitted = mk3s(0.0f);
        uint32_t admitted = 0u, blocked = 0u;
        TraceCounts cnt; cnt.nodes = 0; cnt.tris = 0;
        if (real) {
            const f3 position = pt.position, normal = pt.normal, specular = pt.specular;
            emitted = eye_light(P, pt, rayDirection);                                       // P7
            if (pt.mask == 0u) pt.flags |= RT64_LIGHTING_UNLIT;                             // P4: shade.h:645
            else {
                uint32_t l = 0;
                for (; l < P.lightCount && admitted < RT64_MAX_LIGHTS; l++) {              // shade.h:650-656
                    const RT64_LIGHT L = load_const(P.lights + l);                          // uniform index: scalar loads
                    if (!(pt.mask & L.groupBits)) continue;
                    if (!(light_intensity_simple(L, position, normal, pt.ignoreNormalFactor) > RT_EPSILON)) continue;
                    admitted++;
                    // P5: shade.h:596-632 at lightPointRadius 0, maxSamples 1 (samplePosition = lp, rs = 1)
                    const LightSample ls = light_sample(position, ld_v3(L.position), normal, rayDirection, L, pt.ignoreNormalFactor, pt.specularExponent);
                    const f3 term = ld_v3(L.diffuseColor) * ls.lambert + ld_v3(L.specularColor) * (specular * ls.sp);
                    const float visibility = sample_visibility<CACHED>(P, pt, ls, L, stk, cnt);          // P6
                    if (!(visibility > 0.0f)) blocked++;
                    unshadowed = unshadowed + term;
                    direct = direct + term * visibility;
                }
                if (l < P.lightCount) pt.flags |= RT64_LIGHTING_TRUNCATED;
            }
        }
        keep_counts(P, cnt);
        u32x4 o0, o1, o2, o3;
        o0.x = __float_as_uint(direct.x); o0.y = __float_as_uint(direct.y); o0.z = __float_as_uint(direct.z); o0.w = pt.flags;
        o1.x = __float_as_uint(unshadowed.x); o1.y = __float_as_uint(unshadowed.y); o1.z = __float_as_uint(unshadowed.z); o1.w = admitted;
        o2.x = __float_as_uint(emitted.x); o2.y = __float_as_uint(emitted.y); o2.z = __float_as_uint(emitted.z); o2.w = blocked;
        o3.x = real ? instance : 0xFFFFFFFFu; o3.y = real ? prim : 0xFFFFFFFFu; o3.z = cnt.nodes; o3.w = cnt.tris;
        GOut dst = QUERY_OUT(lighting + i);
        dst[0] = o0; dst[1] = o1; dst[2] = o2; dst[3] = o3;
    }
}

}  // namespace

hipError_t launch_hit_light(const FrameParams &P, const void *rays, const void *hits, const void *lods, void *lighting, uint64_t count, hipStream_t s) {
    decltype(&hit_light_kernel<false>) kernels[2] = { hit_light_kernel<false>, hit_light_kernel<true> };
    return launch_cached(kernels, P, count, 0, s, static_cast<const RT64_RAY *>(rays), static_cast<const RT64_RAY_HIT *>(hits), static_cast<const float *>(lods),
                         static_cast<RT64_RAY_LIGHTING *>(lighting), count);
}
