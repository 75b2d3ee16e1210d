// query_shading.h -- what the ray-query kernels that light a point share: the shaded point of a hit, the eye light, one sample of one light and the shadow walk
// (alpha_query.hip, lighting.hip, sampled_lighting.hip, radiance.hip; rules K5-K7, P2-P7, J2-J9 and W6 in DESIGN.md 4).
//
// Included by query .hip files only, never by shade.h, trace.h, pass_common.h, kernels.h or a frame file: a header the frame kernels compile moves their machine code
// (footprint.hip's head comment has what a lift into shade.h did to 41 of them).  The kernels that call these functions keep their occupancy step, LDS and
// scratch-free frames across the lift (profiles/query_shading_kernel_identity.txt, query_shading_rate.txt).
// The arithmetic restates shade.h: one light is compute_light (:592-633), its shadow ray trace_shadow's; the eye light is direct_light_pixel's tail (passes.hip:299-304).
// Every operation stands in the order the frame has it, so with -ffp-contract=off the values are the frame's bit for bit.
#pragma once
#include "query_common.h"
#include "alpha.h"

// The shaded point of a hit and the material fields a light loop reads.  `flags` are RT64_LIGHTING_* (RT64_SAMPLED_LIGHTING_* are defined as the same bits)
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

// P7 / J9: the point's own light and the eye light (passes.hip:299-304)
DEV f3 eye_light(PRef P, const LightPoint &pt, f3 rayDirection) {
    const float eyeLambert = fmaxf(dot3(pt.normal, -rayDirection), 0.0f);
    const f3 eyeReflected = reflect3(rayDirection, pt.normal);
    const float eyeSpec = s_pow(fmaxf(saturatef(dot3(eyeReflected, -rayDirection)), 0.0f), pt.specularExponent);
    const f3 eyeD = mk3(P.eyeLightDiffuseColor[0], P.eyeLightDiffuseColor[1], P.eyeLightDiffuseColor[2]), eyeS = mk3(P.eyeLightSpecularColor[0], P.eyeLightSpecularColor[1], P.eyeLightSpecularColor[2]);
    return pt.selfLight + (eyeD * eyeLambert + eyeS * (pt.specular * eyeSpec));
}

// P5 / J7: one sample of light L at samplePosition, seen from the point (shade.h:609-621).  The light's term is diffuseColor * lambert + specularColor * (specular * sp)
struct LightSample { f3 direction; float distance, lambert, sp; };
DEV LightSample light_sample(f3 position, f3 samplePosition, f3 normal, f3 rayDirection, const RT64_LIGHT &L, float ignoreNormalFactor, float specularExponent) {
    LightSample r;
    r.distance = len3_exact(position - samplePosition);
    r.direction = normalize3_exact(samplePosition - position);
    const float sampleIntensityFactor = s_pow(fmaxf(1.0f - s_div(r.distance, L.attenuationRadius), 0.0f), L.attenuationExponent);
    const f3 reflectedLight = reflect3(-r.direction, normal);
    const float NdotL = fmaxf(dot3(normal, r.direction), 0.0f);
    r.lambert = lerpf(NdotL, 1.0f, ignoreNormalFactor) * sampleIntensityFactor;
    r.sp = s_pow(fmaxf(saturatef(dot3(reflectedLight, -rayDirection) * sampleIntensityFactor), 0.0f), specularExponent);
    return r;
}

// K5-K7: trace_shadow (shade.h) without a pixel, for a ray the caller has held to Q6 (query_ray_valid): 1 minus the shadow alphas of every intersection in the window,
// 0 at a shadow-opaque instance.  NOISE is J8: the alpha of a caster whose combiner has the noise option is multiplied by noiseFactor (shade.h:538-541).
// The instance differs per lane, and the handler reads it by the frame's `waterfall` (one scalar pass per distinct instance), as trace_shadow does.  In
// alpha_query_kernel's closest-hit handler that form held 2-6 more VGPRs, and on scenes with texture-edge shaders it ignored accepted candidates on about 2 % of the
// rays, so it does not ship there (alpha_query.hip).  That is an OPEN DEFECT, not a settled choice: the cause is not explained (DESIGN.md 4 lists what was ruled
// out), and this handler -- waterfall inside a handler that may return false -- is the same construct; it passes its rules on every case of every kernel that calls
// it, which is evidence, not an explanation.  Whatever is found applies here, once.
// Two things about the signature are measured, not taste (profiles/query_shading_kernel_identity.txt).  The ray comes in as two f3 and the arrays trace_ray wants are
// made here: handed in as arrays, ray_radiance_kernel<true, true> and hit_sampled_light_kernel<true> keep a dead 36-byte spill slot in their frames.  And the Q6 test
// stands in the caller: inside this function visibility_query_kernel took 2-4 more VGPRs and ran about 1 % slower.
template <bool CACHED, bool NOISE = false>
DEV float shadow_visibility(PRef P, f3 origin, f3 direction, float tmin, float tmax, bool cullBackFaces, const TraceStack &stk, TraceCounts &cnt, float noiseFactor = 1.0f) {
    const float o[3] = { origin.x, origin.y, origin.z }, d[3] = { direction.x, direction.y, direction.z };
    float visibility = 1.0f;
    trace_ray<CACHED>(P, o, d, tmin, tmax, cullBackFaces, stk,
                      [&](float, float u, float v, uint32_t instance, uint32_t prim, float &, uint32_t instFlags, float) -> bool {
                          if (instFlags & GPU_INST_SHADOW_OPAQUE) { visibility = 0.0f; return true; }      // K6
                          float sa = 0.0f;
                          waterfall(instance, [&](uint32_t k) {
                              const InstView in = inst_view(P, k);
                              sa = shadow_alpha_before_noise(P, in, prim, u, v);
                              if (NOISE && !(sa < 0.0f) && in.cc.optNoise) sa *= noiseFactor;
                          });
                          if (sa < 0.0f) return false;
                          visibility = fmaxf(visibility - sa, 0.0f);
                          return !(visibility > 0.0f);
                      }, cnt);
    return visibility;
}

// P6 / J8: shade.h:623's ray from the point towards a sample, walked as visibility_query_kernel walks; a ray Q6 refuses is answered 1 without a walk
template <bool CACHED, bool NOISE = false>
DEV float sample_visibility(PRef P, const LightPoint &pt, const LightSample &ls, const RT64_LIGHT &L, const TraceStack &stk, TraceCounts &cnt, float noiseFactor = 1.0f) {
    const float o[3] = { pt.position.x, pt.position.y, pt.position.z }, d[3] = { ls.direction.x, ls.direction.y, ls.direction.z };
    const float tmin = RT_RAY_MIN_DISTANCE + pt.shadowRayBias, tmax = ls.distance - L.shadowOffset;
    if (!query_ray_valid(o, d, tmin, tmax)) return 1.0f;
    return shadow_visibility<CACHED, NOISE>(P, pt.position, ls.direction, tmin, tmax, false, stk, cnt, noiseFactor);
}
