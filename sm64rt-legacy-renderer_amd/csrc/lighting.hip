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
//   The shadow handler is visibility_query_kernel's, statement for statement (alpha_query.hip; its head comment has the open defect of the `waterfall` form).
// The arithmetic restates shade.h: light_intensity_simple (:581-589) is called; one light is compute_light (:592-633) with radius 0 and one sample, the visibility
// kept apart from the term so that `unshadowed` and `direct` come from the same numbers; `emitted` is direct_light_pixel's tail (passes.hip:299-304).
#include "query_common.h"
#include "alpha.h"

namespace {

struct LightPoint { f3 position, normal, specular, selfLight; float ignoreNormalFactor, shadowRayBias, specularExponent; uint32_t mask, flags; };

// P2 and the material fields of P4-P7 for one real hit of instance `in`: surface_of_hit's position, material_of_hit's normal chain and specular texel
DEV void point_of_hit(PRef P, const InstView &in, uint32_t prim, float u, float v, f3 rayDirW, float lod, LightPoint &r) {
    const GpuCombiner &cc = in.cc;
    const RT64_MATERIAL &mat = in.material;
    const bool normalMap = (in.flags & GPU_INST_NORMAL_MAP) != 0, specularMap = (in.flags & GPU_INST_SPECULAR_MAP) != 0;
    const float b[3] = { 1.0f - u - v, u, v };
    VertexData vd;
    get_vertex_data(in, prim, b, cc.vertexUV && normalMap, vd);
    r.flags = RT64_LIGHTING_VALID;
    r.position = mul_point(in.objectToWorld.m, vd.vertexPosition);                          // A4
    f3 vertexNormal = normalize3(mul_vector(in.objectToWorldNormal.m, vd.vertexNormal));    // H8
    const bool back = dot3(vd.triangleNormal, rayDirW) > 0.0f;
    const float normalSign = back ? -1.0f : 1.0f;
    if (back) r.flags |= RT64_LIGHTING_BACK_FACE;
    vertexNormal = vertexNormal * normalSign;
    float unused;
    if (cc.vertexUV && normalMap && in.texNormal >= 0) {
        const f3 tangent = normalize3(mul_vector(in.objectToWorldNormal.m, vd.vertexTangent)) * normalSign;
        const f3 binormal = normalize3(mul_vector(in.objectToWorldNormal.m, vd.vertexBinormal)) * normalSign;
        const float s = mat.uvDetailScale;
        const f4 tex = tex_sample_lod(tex_view(P.textures + in.texNormal), vd.vertexUV.x * s, vd.vertexUV.y * s, lod, in.filter, in.hAddr, in.vAddr, unused);
        const f3 nc = mk3(tex.x * 2.0f - 1.0f, tex.y * 2.0f - 1.0f, tex.z * 2.0f - 1.0f);
        vertexNormal = normalize3((vertexNormal * nc.z + tangent * nc.x) + binormal * nc.y);
    }
    r.normal = vertexNormal;
    r.specular = mk3s(1.0f);                                                                // H9
    if (cc.vertexUV && specularMap && in.texSpecular >= 0) {
        const float s = mat.uvDetailScale;
        const f4 tex = tex_sample_lod(tex_view(P.textures + in.texSpecular), vd.vertexUV.x * s, vd.vertexUV.y * s, lod, in.filter, in.hAddr, in.vAddr, unused);
        r.specular = xyz(tex);
    }
    r.selfLight = ld_v3(mat.selfLight);
    r.ignoreNormalFactor = mat.ignoreNormalFactor; r.shadowRayBias = mat.shadowRayBias; r.specularExponent = mat.specularExponent;
    r.mask = mat.lightGroupMaskBits;
}

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
            {                                                                               // P7: passes.hip:299-304
                const float eyeLambert = fmaxf(dot3(normal, -rayDirection), 0.0f);
                const f3 eyeReflected = reflect3(rayDirection, normal);
                const float eyeSpec = s_pow(fmaxf(saturatef(dot3(eyeReflected, -rayDirection)), 0.0f), pt.specularExponent);
                const f3 eyeD = mk3(P.eyeLightDiffuseColor[0], P.eyeLightDiffuseColor[1], P.eyeLightDiffuseColor[2]), eyeS = mk3(P.eyeLightSpecularColor[0], P.eyeLightSpecularColor[1], P.eyeLightSpecularColor[2]);
                emitted = pt.selfLight + (eyeD * eyeLambert + eyeS * (specular * eyeSpec));
            }
            if (pt.mask == 0u) pt.flags |= RT64_LIGHTING_UNLIT;                             // P4: shade.h:645
            else {
                uint32_t l = 0;
                for (; l < P.lightCount && admitted < RT64_MAX_LIGHTS; l++) {              // shade.h:650-656
                    const RT64_LIGHT L = load_const(P.lights + l);                          // uniform index: scalar loads
                    if (!(pt.mask & L.groupBits)) continue;
                    if (!(light_intensity_simple(L, position, normal, pt.ignoreNormalFactor) > RT_EPSILON)) continue;
                    admitted++;
                    // P5: shade.h:596-632 at lightPointRadius 0, maxSamples 1 (samplePosition = lp, rs = 1)
                    const f3 lp = ld_v3(L.position);
                    const float sampleDistance = len3_exact(position - lp);
                    const f3 sampleDirection = normalize3_exact(lp - position);
                    const float sampleIntensityFactor = s_pow(fmaxf(1.0f - s_div(sampleDistance, L.attenuationRadius), 0.0f), L.attenuationExponent);
                    const f3 reflectedLight = reflect3(-sampleDirection, normal);
                    const float NdotL = fmaxf(dot3(normal, sampleDirection), 0.0f);
                    const float sampleLambert = lerpf(NdotL, 1.0f, pt.ignoreNormalFactor) * sampleIntensityFactor;
                    const float sp = s_pow(fmaxf(saturatef(dot3(reflectedLight, -rayDirection) * sampleIntensityFactor), 0.0f), pt.specularExponent);
                    const f3 term = ld_v3(L.diffuseColor) * sampleLambert + ld_v3(L.specularColor) * (specular * sp);
                    // P6: shade.h:623's ray, walked as visibility_query_kernel walks (K5-K7)
                    const float o[3] = { position.x, position.y, position.z }, d[3] = { sampleDirection.x, sampleDirection.y, sampleDirection.z };
                    const float tmin = RT_RAY_MIN_DISTANCE + pt.shadowRayBias, tmax = sampleDistance - L.shadowOffset;
                    float visibility = 1.0f;
                    if (query_ray_valid(o, d, tmin, tmax)) {
                        trace_ray<CACHED>(P, o, d, tmin, tmax, false, stk,
                                          [&](float, float hu, float hv, uint32_t hitInstance, uint32_t hitPrim, float &, uint32_t instFlags, float) -> bool {
                                              if (instFlags & GPU_INST_SHADOW_OPAQUE) { visibility = 0.0f; return true; }      // K6
                                              float sa = 0.0f;
                                              waterfall(hitInstance, [&](uint32_t k) { sa = shadow_alpha_before_noise(P, inst_view(P, k), hitPrim, hu, hv); });
                                              if (sa < 0.0f) return false;
                                              visibility = fmaxf(visibility - sa, 0.0f);
                                              return !(visibility > 0.0f);
                                          }, cnt);
                    }
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
    if (!count) return hipSuccess;
    const dim3 grid = query_grid(count), block(RT_BLOCK);
    const RT64_RAY *r = static_cast<const RT64_RAY *>(rays); const RT64_RAY_HIT *h = static_cast<const RT64_RAY_HIT *>(hits);
    const float *l = static_cast<const float *>(lods); RT64_RAY_LIGHTING *o = static_cast<RT64_RAY_LIGHTING *>(lighting);
    if (P.cacheWords) hipLaunchKernelGGL((hit_light_kernel<true>), grid, block, (size_t)P.cacheWords * 16, s, P, r, h, l, o, count);
    else hipLaunchKernelGGL((hit_light_kernel<false>), grid, block, 0, s, P, r, h, l, o, count);
    return hipGetLastError();
}
