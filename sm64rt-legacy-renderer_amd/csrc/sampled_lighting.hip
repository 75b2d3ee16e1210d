// sampled_lighting.hip -- the direct light of a query's hits as a frame's pixel samples it (RT64_SampleViewRayLights, include/rt64_sampled_lighting.h; rules J1-J11 in DESIGN.md 4).
//
// hit_light_kernel (lighting.hip) with the frame's draws put back: per record it reads 80 bytes (ray + hit + key, 16-byte loads; without keys the key is the
// record's place in the frame) and one optional float (the lod), rebuilds the shaded point as hit_light_kernel does (J2), scans the candidates into this lane's
// LDS columns (J5), draws min(candidates, maxLights) of them with the key's blue noise (J6), samples max(diSamples, 1) points of each drawn light's disc (J7) and
// walks one shadow ray per sample (J8).  It writes 64 bytes (four 16-byte stores).
//   fill_cache / lane_stack / use_cache and the spill slab are the walk kernels'; load_ray / load_hit the resolve kernels'; the hit's own instance is read by
//   material.hip's scheme (scalar loads for a wave whose hits agree on it, per-lane inst_view otherwise), as in lighting.hip.
//   The candidate columns (sLightIntensities / sLightIndices of Lights.hlsli:121-122) are indexed by the slot a lane's random number picks, so they live in LDS, not
//   in registers or scratch: [wave][slot][lane] floats, then [wave][slot][lane] bytes, in dynamic LDS behind the cache image, slots = min(lights of the frame, 16) + 1
//   as pass_common.h's light_slots sizes them for the frame kernels.  A float access is one ds instruction whose lanes sit on 64 consecutive words whatever slot each
//   lane asks for; the bytes of a slot share 16 words, four lanes a word.
//   The drawn light differs per lane: it is fetched by shade.h's `waterfall`, one scalar pass per distinct light of the wave, as compute_light does (shade.h:595).
//   The shaded point, the eye light, the light sample and the shadow walk are query_shading.h's, the copy hit_light_kernel calls; the walk is its NOISE form, J8's
//   factor applied to the alpha of a caster whose combiner has the noise option (shade.h:538-541; shadow_visibility has the open defect of its `waterfall` handler).
// The arithmetic restates shade.h with the key (x, y, frame) for (px, py, P.frameCount): compute_lights_random (:636-672) and the disc of compute_light (:594-608), the
// shadow term kept apart from the light's term so that `unshadowed` and `direct` come from the same numbers; light_intensity_simple, blue_noise, init_rand and
// next_rand are called.
#include "query_shading.h"

namespace {

// slots of a lane's candidate columns: pass_common.h's light_slots
DEV uint32_t column_slots(PRef P) { return (P.lightCount < RT64_MAX_LIGHTS ? P.lightCount : (uint32_t)RT64_MAX_LIGHTS) + 1u; }

// keys == nullptr: record i of the launch is record first + i of the call, keyed by its place in the frame (J3)
template <bool CACHED>
__global__ __launch_bounds__(RT_BLOCK) void hit_sampled_light_kernel(FrameParams Pv, const RT64_RAY *rays, const RT64_RAY_HIT *hits, const float *lods, const RT64_LIGHT_SAMPLE_KEY *keys,
                                                                     uint64_t first, uint32_t maxLights, uint32_t diSamples, RT64_RAY_SAMPLED_LIGHTING *records, uint64_t count) {
    PRef P = *kernel_params(); (void)Pv;
    __shared__ uint32_t ldsStack[QUERY_STACK_WORDS(CACHED) * RT_BLOCK];
    extern __shared__ u32x4_lds dynLds[];
    fill_cache<CACHED>(P, dynLds);
    TraceStack stk = lane_stack<CACHED>(P, ldsStack);
    if (CACHED) stk.use_cache(dynLds);
    // this lane's candidate columns, [wave][slot][lane], behind the cache image
    const uint32_t slots = column_slots(P);
    float *const columns = reinterpret_cast<float *>(dynLds + (CACHED ? P.cacheWords : 0u));
    const uint32_t column = (threadIdx.x >> 6) * slots * RT_LANES + (threadIdx.x & 63u);
    float *const sInt = columns + column;
    uint8_t *const sIdx = reinterpret_cast<uint8_t *>(columns + slots * RT_BLOCK) + column;
    const uint64_t stride = query_stride();
    for (uint64_t i = query_first(); i < count; i += stride) {
        const QueryRay ray = load_ray(QUERY_IN(rays + i));          // (a record does not depend on the origin: that load is dead code)
        const QueryHit h = load_hit(QUERY_IN(hits + i));
        const float lod = lods ? load_global(lods + i) : 0.0f;
        uint32_t kx, ky, kf;                                                // J3
        if (keys) { const u32x4 k = QUERY_IN(keys + i)[0]; kx = k.x; ky = k.y; kf = k.z; }
        else { const uint64_t at = first + i; const uint32_t w = (uint32_t)P.width; kx = (uint32_t)(at % w); ky = (uint32_t)(at / w); kf = P.frameCount; }
        const f3 rayDirection = mk3(ray.d[0], ray.d[1], ray.d[2]);          // J2: as given
        const uint32_t instance = h.instance, prim = h.prim;
        const float u = h.u, v = h.v;
        // J1: the miss record; nothing below reads through an index that is out of range
        LightPoint pt;
        pt.position = pt.normal = pt.specular = pt.selfLight = mk3s(0.0f); pt.ignoreNormalFactor = pt.shadowRayBias = pt.specularExponent = 0.0f; pt.mask = 0u;
        pt.flags = (int32_t)instance < 0 ? 0u : (uint32_t)RT64_SAMPLED_LIGHTING_BAD_HIT;
        bool real = false;
        if (instance < P.instanceCount) {               // (unsigned: a negative instance is past the end)
            const uint32_t k0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)instance);
            if (__ballot(instance != k0) == 0ull) {     // the lanes in here agree: k0 is wave-uniform, inst_view's loads are scalar and the map branches uniform
                if (prim < load_const(&P.instances[k0].triCount)) { point_of_hit(P, inst_view(P, k0), prim, u, v, rayDirection, lod, pt); real = true; }
            }
            else if (prim < load_const(&P.instances[instance].triCount)) { point_of_hit(P, inst_view(P, instance), prim, u, v, rayDirection, lod, pt); real = true; }
        }
        f3 direct = mk3s(0.0f), unshadowed = mk3s(0.0f), emitted = mk3s(0.0f);
        uint32_t sCount = 0u, drawn = 0u;
        TraceCounts cnt; cnt.nodes = 0; cnt.tris = 0;
        if (real) {
            const f3 position = pt.position, normal = pt.normal, specular = pt.specular;
            emitted = eye_light(P, pt, rayDirection);                                       // J9
            if (pt.mask == 0u) pt.flags |= RT64_SAMPLED_LIGHTING_UNLIT;                     // J5: shade.h:645
            else {
                float total = 0.0f;
                uint32_t l = 0;
                for (; l < P.lightCount && sCount < RT64_MAX_LIGHTS; l++) {                // shade.h:650-656
                    const RT64_LIGHT Ll = load_const(P.lights + l);                         // uniform index: scalar loads
                    if (!(pt.mask & Ll.groupBits)) continue;
                    const float li = light_intensity_simple(Ll, position, normal, pt.ignoreNormalFactor);
                    if (li > RT_EPSILON) { sInt[sCount * RT_LANES] = li; sIdx[sCount * RT_LANES] = (uint8_t)l; total += li; sCount++; }
                }
                if (l < P.lightCount) pt.flags |= RT64_SAMPLED_LIGHTING_TRUNCATED;
                // J8's factor: one number per key (shade.h:539-540)
                uint32_t seed = init_rand(kx + ky * (uint32_t)P.width, kf, 16);
                const float noiseFactor = rintf(next_rand(seed));
                const bool single = sCount == 1u && maxLights >= 1u;                        // shade.h:657: chosen whatever the random number is, with probability 1
                float randomRange = total;
                const uint32_t lCount = sCount < maxLights ? sCount : maxLights;
                const bool useProbability = lCount == 1u;
                for (uint32_t s = 0; s < lCount; s++) {                                     // J6: shade.h:662-670
                    uint32_t chosen = 0; float invProbability = 1.0f;
                    if (!single) {
                        const float r = blue_noise(P, kx, ky, kf + s).x * randomRange;
                        float rInt = sInt[0];
                        while (chosen < sCount - 1u && r >= rInt) { chosen++; rInt += sInt[chosen * RT_LANES]; }
                        const float cInt = sInt[chosen * RT_LANES];
                        if (useProbability) invProbability = s_div(randomRange, cInt);
                        sInt[chosen * RT_LANES] = 0.0f; randomRange -= cInt;
                    }
                    const uint32_t cIdx = sIdx[chosen * RT_LANES];
                    drawn |= (drawn & (1u << chosen)) ? (0x10000u << chosen) : (1u << chosen);
                    // J7: shade.h:594-632
                    RT64_LIGHT L;
                    waterfall(cIdx, [&](uint32_t k) { L = load_const(P.lights + k); });      // one scalar fetch per distinct light chosen in the wave
                    const f3 lp = ld_v3(L.position);
                    const f3 lightDirection = normalize3(lp - position);
                    const float lightPointRadius = (diSamples > 0u) ? L.pointRadius : 0.0f;
                    f3 perpX = cross3(-lightDirection, mk3(0.0f, 1.0f, 0.0f));
                    if (perpX.x == 0.0f && perpX.y == 0.0f && perpX.z == 0.0f) perpX.x = 1.0f;
                    const f3 perpY = cross3(perpX, -lightDirection);
                    const uint32_t maxSamples = diSamples > 1u ? diSamples : 1u;
                    const float rs = s_rcp((float)maxSamples);
                    float lLambert = 0.0f, lShadow = 0.0f; f3 lSpec = mk3s(0.0f);
                    for (uint32_t samples = maxSamples; samples > 0u; samples--) {
                        f3 samplePosition = lp;          // radius 0: the disc offsets are finite numbers times 0 (shade.h:605-608)
                        if (lightPointRadius != 0.0f || !(lightDirection.x == lightDirection.x)) {
                            const f3 bn = blue_noise(P, kx, ky, kf + samples);
                            float scx = bn.x * 2.0f - 1.0f, scy = bn.y * 2.0f - 1.0f;
                            const float len = s_sqrt(scx * scx + scy * scy), sat = saturatef(len), rlen = s_rcp(len);
                            scx = scx * rlen * sat; scy = scy * rlen * sat;
                            samplePosition = (lp + (perpX * scx) * lightPointRadius) + (perpY * scy) * lightPointRadius;
                        }
                        const LightSample ls = light_sample(position, samplePosition, normal, rayDirection, L, pt.ignoreNormalFactor, pt.specularExponent);
                        const float visibility = sample_visibility<CACHED, true>(P, pt, ls, L, stk, cnt, noiseFactor);          // J8: the caster's noise included
                        lLambert += ls.lambert * rs;
                        lSpec = lSpec + (specular * ls.sp) * rs;
                        lShadow += visibility * rs;
                    }
                    const f3 term = ld_v3(L.diffuseColor) * lLambert + ld_v3(L.specularColor) * lSpec;
                    unshadowed = unshadowed + term * invProbability;
                    direct = direct + (term * lShadow) * invProbability;
                }
            }
        }
        keep_counts(P, cnt);
        u32x4 o0, o1, o2, o3;
        o0.x = __float_as_uint(direct.x); o0.y = __float_as_uint(direct.y); o0.z = __float_as_uint(direct.z); o0.w = pt.flags;
        o1.x = __float_as_uint(unshadowed.x); o1.y = __float_as_uint(unshadowed.y); o1.z = __float_as_uint(unshadowed.z); o1.w = sCount;
        o2.x = __float_as_uint(emitted.x); o2.y = __float_as_uint(emitted.y); o2.z = __float_as_uint(emitted.z); o2.w = drawn;
        o3.x = real ? instance : 0xFFFFFFFFu; o3.y = real ? prim : 0xFFFFFFFFu; o3.z = cnt.nodes; o3.w = cnt.tris;
        GOut dst = QUERY_OUT(records + i);
        dst[0] = o0; dst[1] = o1; dst[2] = o2; dst[3] = o3;
    }
}

}  // namespace

hipError_t launch_hit_sampled_light(const FrameParams &P, const void *rays, const void *hits, const void *lods, const void *keys, uint64_t first, uint32_t maxLights, uint32_t diSamples,
                                    void *records, uint64_t count, hipStream_t s) {
    decltype(&hit_sampled_light_kernel<false>) kernels[2] = { hit_sampled_light_kernel<false>, hit_sampled_light_kernel<true> };
    // the candidate columns behind the cache image: slots x RT_BLOCK floats, then slots x RT_BLOCK bytes
    const size_t slots = (P.lightCount < RT64_MAX_LIGHTS ? P.lightCount : (uint32_t)RT64_MAX_LIGHTS) + 1u, columns = slots * RT_BLOCK * (sizeof(float) + 1);
    return launch_cached(kernels, P, count, columns, s, static_cast<const RT64_RAY *>(rays), static_cast<const RT64_RAY_HIT *>(hits), static_cast<const float *>(lods),
                         static_cast<const RT64_LIGHT_SAMPLE_KEY *>(keys), first, maxLights, diSamples, static_cast<RT64_RAY_SAMPLED_LIGHTING *>(records), count);
}
