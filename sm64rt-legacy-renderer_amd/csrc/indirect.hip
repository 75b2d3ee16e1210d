// indirect.hip -- the indirect light of a point as a frame's pixel samples it (RT64_GenerateViewPointGIRays, RT64_ComposeViewGIRays, RT64_TraceViewPointsIndirect,
// RT64_TraceViewRayIndirect, include/rt64_indirect.h; rules Y1-Y12 in DESIGN.md 4).
//
// The frame's GI pass (indirect_kernel of passes.hip) as a chain of small kernels of query_common.h, for the reason passes.hip gives at "IndirectRayGen as a wavefront
// pair": bounce walk, any-hit, texturing, light pick and shadow walk in one kernel are 237 VGPRs.  The walk between the links is layers.hip's layer_walk_kernel, unchanged.
//   gi_ray_kernel            a resolve kernel, no LDS: per ray 32 bytes in (position and normal: two 16-byte loads), the key (16 bytes, or the ray's place in the frame),
//                            cos_hemisphere_blue_noise of shade.h -- called, not restated -- and two 16-byte stores.  The source records are RT64_GI_POINTs (one per
//                            point, shared by the point's samples) or, for a second bounce, the RT64_GI_SAMPLEs of the first (one per ray): position word and normal word
//                            are neighbours in both.
//   gi_shade_kernel<LIGHT, CACHED>  a resolve kernel that also walks, ray_radiance_kernel's shape: fill_cache / lane_stack / use_cache and the spill slab are the walk
//                            kernels'.  Per ray the loop of indirect_kernel ("for (uint32_t hit = 0; hit < nhits; hit++)") over records (l, i) at l count + i, so that
//                            neighbouring lanes read neighbouring records; the instance of a layer is read by material.hip's scheme (scalar loads for a wave whose lanes
//                            agree on it, per-lane inst_view otherwise).  Per-lane state: the running colour and coverage, the last contributing layer's index and its
//                            hit (instance, primitive, t, u, v): the LightPoint is built from those ONCE, after the loop.  No per-lane array is indexed by a run-time
//                            value: the candidate columns of the light draw live in LDS, [wave][slot][lane], behind the cache image, as in sampled_lighting.hip.
//                            LIGHT = false is the resolve alone (the chain needs the first bounce's position and normal before it can send the second): no walk, hence
//                            no stack, no scene cache and no LDS at all; radiance is 0.
//   gi_point_kernel          a resolve kernel, no LDS: the hit of a ray -> the RT64_GI_POINT RT64_TraceViewRayIndirect starts from (point_of_hit of query_shading.h).
//   gi_accumulate_kernel     a resolve kernel, no LDS: per point the frame's running mean and luminance moments over its samples' records, three 16-byte stores.
// What is restated.  gi_layer_colour is radiance.hip's layer_colour at level 0 (a bounce ray carries no differentials: the frame's gradient sample with zero gradients
// and tex_sample_lod at lod 0 run the same statements) with the one thing a frame's surface any-hit has besides: the noise option of the shader, keyed by the record's
// key instead of the pixel (shade.h, surface_anyhit_view: "if (cc.optNoise)").  radiance.hip says why that function is not shared; a third caller does not change it.
// The single light draw is sampled_lighting.hip's draw loop for maxLights = 1, instantiated here: lifted into a header, hit_sampled_light_kernel would have to compile
// to the same machine code to stay what its profiles describe, and nothing but a compile of both shows that.
// What is shared.  The shaded point (point_of_hit), the light sample and the shadow walk with noise casters are query_shading.h's; blue_noise, init_rand, next_rand,
// light_intensity_simple, sky_over_background_envmap and cos_hemisphere_blue_noise are shade.h's.
// Every operation stands in the order indirect_kernel has it, so with -ffp-contract=off the values are the frame's; the Makefile compiles this file without the SLP
// vectorizer, as radiance.hip and sampled_lighting.hip.
#include "query_shading.h"
#include "../../include/rt64_indirect.h"

namespace {

// the key of record `at` of the call: keys[at], or its place in the frame (J3)
struct GiKey { uint32_t x, y, frame; };

// Y1: what of a source record makes a point to start a ray from.  a: position + flags, b: normal + instance
DEV bool gi_point_usable(const u32x4 &a, const u32x4 &b, uint32_t needFlags, uint32_t refuseFlags) {
    const float px = __uint_as_float(a.x), py = __uint_as_float(a.y), pz = __uint_as_float(a.z), nx = __uint_as_float(b.x), ny = __uint_as_float(b.y), nz = __uint_as_float(b.z);
    bool ok = (a.w & needFlags) == needFlags && (a.w & refuseFlags) == 0u && (nx != 0.0f || ny != 0.0f || nz != 0.0f);
    ok = ok && __builtin_isfinite(px) && __builtin_isfinite(py) && __builtin_isfinite(pz) && __builtin_isfinite(nx) && __builtin_isfinite(ny) && __builtin_isfinite(nz);
    return ok;
}

// Ray i of the launch belongs to point i % points and is sample slot slotTop - i / points of it (the chain lays the rays of a chunk out sample-major; a public call has
// points = count: ray i, point i, slot slotTop).  A launch whose points < count has fewer than 2^32 rays (the host bounds a chunk), so the division is 32 bits wide.
DEV void gi_ray_place(uint64_t i, uint64_t points, uint64_t count, uint64_t &point, uint32_t &sample) {
    point = i; sample = 0u;
    if (points < count) { sample = (uint32_t)i / (uint32_t)points; point = (uint32_t)i - sample * (uint32_t)points; }
}

// src: 16-byte words; the position word of source record r is src[r * strideWords], its normal word the next one.  perRay: source record i belongs to ray i (a second
// bounce's), otherwise to the ray's point.
__global__ __launch_bounds__(RT_BLOCK) void gi_ray_kernel(FrameParams Pv, const u32x4 *src, uint32_t strideWords, uint32_t perRay, uint32_t needFlags, uint32_t refuseFlags,
                                                          const RT64_LIGHT_SAMPLE_KEY *keys, uint64_t first, uint64_t points, uint32_t giSamples, uint32_t slotTop, uint32_t second,
                                                          RT64_RAY *rays, uint64_t count) {
    PRef P = *kernel_params(); (void)Pv;
    const uint64_t stride = query_stride();
    const uint32_t mult = 64u / giSamples;                                  // (the host refused giSamples = 0)
    const uint32_t step = second ? (mult > 1u ? mult / 2u : 1u) : 0u;      // I9
    for (uint64_t i = query_first(); i < count; i += stride) {
        uint64_t point; uint32_t sample;
        gi_ray_place(i, points, count, point, sample);
        const uint64_t r = perRay ? i : point;
        const GIn in = QUERY_IN(src + r * strideWords);
        const u32x4 a = in[0], b = in[1];
        uint32_t kx, ky, kf;                                                // Y2
        if (keys) { const u32x4 k = QUERY_IN(keys + point)[0]; kx = k.x; ky = k.y; kf = k.z; }
        else { const uint64_t at = first + point; const uint32_t w = (uint32_t)P.width; kx = (uint32_t)(at % w); ky = (uint32_t)(at / w); kf = P.frameCount; }
        u32x4 o0, o1;
        o0.x = o0.y = o0.z = o0.w = 0u; o1 = o0;                            // Y4: the ray every walk answers with a miss
        if (gi_point_usable(a, b, needFlags, refuseFlags)) {
            const f3 normal = mk3(__uint_as_float(b.x), __uint_as_float(b.y), __uint_as_float(b.z));
            const uint32_t slot = slotTop - sample;
            const f3 d = cos_hemisphere_blue_noise(P, kx, ky, kf + slot * mult + step, normal);      // passes.hip: P.frameCount + maxSamples * blueNoiseMult (+ the second bounce's step)
            o0.x = a.x; o0.y = a.y; o0.z = a.z; o0.w = __float_as_uint(RT_RAY_MIN_DISTANCE);
            o1.x = __float_as_uint(d.x); o1.y = __float_as_uint(d.y); o1.z = __float_as_uint(d.z); o1.w = __float_as_uint(RT_RAY_MAX_DISTANCE);
        }
        GOut dst = QUERY_OUT(rays + i);
        dst[0] = o0; dst[1] = o1;
    }
}

// radiance.hip's layer_colour at level 0, with the surface any-hit's noise option (shade.h, surface_anyhit_view): the same calls in the same order.  false: a texture-edge
// shader cuts the intersection out (the walk has dropped those already: K2).
DEV bool gi_layer_colour(PRef P, const InstView &in, uint32_t prim, float u, float v, float noiseFactor, f4 &colour) {
    const GpuCombiner &cc = in.cc;
    const RT64_MATERIAL &mat = in.material;
    const float b[3] = { 1.0f - u - v, u, v };
    const f4 mix = mk4(mat.diffuseColorMix.x, mat.diffuseColorMix.y, mat.diffuseColorMix.z, mat.diffuseColorMix.w);
    VertexData vd;
    get_vertex_data(in, prim, b, false, vd);
    f4 t0 = mk4(0, 0, 0, 0);
    const f4 t1 = mk4(1.0f, 0.0f, 1.0f, 1.0f);
    if (cc.useTex0) {
        float unused;
        const f4 tex = tex_sample_lod(tex_view(P.textures + in.texDiffuse), vd.vertexUV.x, vd.vertexUV.y, 0.0f, in.filter, in.hAddr, in.vAddr, unused);
        const float k = fmaxf(-mix.w, 0.0f);
        t0 = mk4(lerpf(tex.x, mix.x, k), lerpf(tex.y, mix.y, k), lerpf(tex.z, mix.z, k), tex.w);
    }
    f4 result;
    if (!cc.colorAlphaSame && cc.optAlpha) {
        result = color_formula(cc, false, true, vd, t0, t1);
        result.w = alpha_formula(cc, vd, t0, t1);
    }
    else result = color_formula(cc, cc.optAlpha, cc.optAlpha, vd, t0, t1);
    {
        const float k = fmaxf(mix.w, 0.0f);
        result.x = lerpf(result.x, mix.x, k); result.y = lerpf(result.y, mix.y, k); result.z = lerpf(result.z, mix.z, k);
    }
    result.w = clampf(mat.solidAlphaMultiplier * result.w, 0.0f, 1.0f);
    if (cc.optTextureEdge) { if (result.w > RT64_EDGE_ALPHA) result.w = 1.0f; else return false; }
    if (cc.optNoise) result.w *= noiseFactor;
    colour = mk4(q_unorm8(result.x), q_unorm8(result.y), q_unorm8(result.z), q_unorm8(result.w));      // shade.h: rec.color
    return true;
}

// The running sums of indirect_kernel's loop (Y5)
struct GiResolve { f3 rgb; float rem; int lit; uint32_t layers, flags; };

// The body of indirect_kernel's loop for one real hit of instance `in`
DEV void gi_layer_step(PRef P, const InstView &in, const QueryHit &h, uint32_t l, float noiseFactor, GiResolve &s) {
    f4 hitColor;
    if (!gi_layer_colour(P, in, h.prim, h.u, h.v, noiseFactor, hitColor)) return;      // passes.hip: `if (!surface_record(...)) continue;`
    const float alphaContrib = s.rem * hitColor.w;
    if (alphaContrib >= RT_EPSILON) {
        s.rgb.x += hitColor.x * alphaContrib; s.rgb.y += hitColor.y * alphaContrib; s.rgb.z += hitColor.z * alphaContrib;
        s.rem *= (1.0f - hitColor.w);
        s.lit = (int)l;
        s.layers++;
    }
    if (s.rem <= RT_EPSILON) s.flags |= RT64_GI_SAMPLE_COVERED;
}

// Y5: the surface the resolve ended on, as the frame's hit record holds it: position along the ray, SNORM16 normal, specularColor times the UNORM8 specular texel
DEV void gi_point_of_layer(PRef P, const InstView &in, uint32_t prim, float t, float u, float v, f3 rayOrigin, f3 rayDirection, LightPoint &pt) {
    point_of_hit(P, in, prim, u, v, rayDirection, 0.0f, pt);
    const RT64_MATERIAL &m = in.material;
    const float dist = t - m.depthBias;                                                 // shade.h: rec.dist
    pt.position = rayOrigin + rayDirection * (dist + m.depthBias);                      // passes.hip: resPosition
    pt.normal = mk3(q_snorm16(pt.normal.x), q_snorm16(pt.normal.y), q_snorm16(pt.normal.z));
    pt.specular = ld_v3(m.specularColor) * mk3(q_unorm8(pt.specular.x), q_unorm8(pt.specular.y), q_unorm8(pt.specular.z));
}

// incoming: 3 floats per ray at incoming[i * incomingStride], or nullptr.  keys, first, points: as gi_ray_kernel's.
template <bool LIGHT, bool CACHED>
__global__ __launch_bounds__(RT_BLOCK) void gi_shade_kernel(FrameParams Pv, const RT64_RAY *rays, const RT64_RAY_HIT *hits, const RT64_LIGHT_SAMPLE_KEY *keys, uint64_t first, uint64_t points,
                                                            const float *incoming, uint32_t incomingStride, uint32_t diSamples, RT64_GI_SAMPLE *samples, uint64_t count, uint32_t maxLayers) {
    PRef P = *kernel_params(); (void)Pv;
    __shared__ uint32_t ldsStack[LIGHT ? QUERY_STACK_WORDS(CACHED) * RT_BLOCK : 1];
    extern __shared__ u32x4_lds dynLds[];
    TraceStack stk;
    float *sInt = nullptr; uint8_t *sIdx = nullptr;
    if (LIGHT) {
        fill_cache<CACHED>(P, dynLds);
        stk = lane_stack<CACHED>(P, ldsStack);
        if (CACHED) stk.use_cache(dynLds);
        // this lane's candidate columns, [wave][slot][lane], behind the cache image (sampled_lighting.hip)
        const uint32_t slots = (P.lightCount < RT64_MAX_LIGHTS ? P.lightCount : (uint32_t)RT64_MAX_LIGHTS) + 1u;
        float *const columns = reinterpret_cast<float *>(dynLds + (CACHED ? P.cacheWords : 0u));
        const uint32_t column = (threadIdx.x >> 6) * slots * RT_LANES + (threadIdx.x & 63u);
        sInt = columns + column;
        sIdx = reinterpret_cast<uint8_t *>(columns + slots * RT_BLOCK) + column;
    }
    const uint64_t stride = query_stride();
    for (uint64_t i = query_first(); i < count; i += stride) {
        PRef P = *kernel_params_here();      // this trip's view of the frame constants (radiance.hip says what carrying them across the trips costs)
        const f3 ambientBase = mk3(P.ambientBaseColor[0], P.ambientBaseColor[1], P.ambientBaseColor[2]);
        const QueryRay ray = load_ray(QUERY_IN(rays + i));
        uint64_t point; uint32_t sample;
        gi_ray_place(i, points, count, point, sample);
        uint32_t kx, ky, kf;                                                // Y2
        if (keys) { const u32x4 k = QUERY_IN(keys + point)[0]; kx = k.x; ky = k.y; kf = k.z; }
        else { const uint64_t at = first + point; const uint32_t w = (uint32_t)P.width; kx = (uint32_t)(at % w); ky = (uint32_t)(at / w); kf = P.frameCount; }
        const bool valid = query_ray_valid(ray.o, ray.d, ray.tmin, ray.tmax);
        const f3 rayOrigin = mk3(ray.o[0], ray.o[1], ray.o[2]), rayDirection = mk3(ray.d[0], ray.d[1], ray.d[2]);          // as given
        // one number per key: the noise option of a surface shader (shade.h:482-485) and of a shadow caster (:538-541)
        uint32_t seed = init_rand(kx + ky * (uint32_t)P.width, kf, 16);
        const float noiseFactor = rintf(next_rand(seed));
        GiResolve st;
        st.rgb = mk3s(0.0f); st.rem = 1.0f; st.lit = -1; st.layers = 0u; st.flags = valid ? (uint32_t)RT64_GI_SAMPLE_VALID : 0u;
        uint32_t litInstance = 0u, litPrim = 0u; float litT = 0.0f, litU = 0.0f, litV = 0.0f;
        const uint32_t listed = valid ? maxLayers : 0u;          // a Q6-invalid ray reads no record
        for (uint32_t l = 0; l < listed; l++) {
            const QueryHit h = load_hit(QUERY_IN(hits + ((uint64_t)l * count + i)));
            if ((int32_t)h.instance < 0) break;                                             // the list's end
            bool real = false;
            if (h.instance < P.instanceCount) {
                const uint32_t k0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)h.instance);
                if (__ballot(h.instance != k0) == 0ull) {       // the lanes in here agree: k0 is wave-uniform, inst_view's loads are scalar and the combiner's branches uniform
                    if (h.prim < load_const(&P.instances[k0].triCount)) { gi_layer_step(P, inst_view(P, k0), h, l, noiseFactor, st); real = true; }
                }
                else if (h.prim < load_const(&P.instances[h.instance].triCount)) { gi_layer_step(P, inst_view(P, h.instance), h, l, noiseFactor, st); real = true; }
            }
            if (!real) { st.flags |= RT64_GI_SAMPLE_BAD_HIT; break; }
            if (st.lit == (int)l) { litInstance = h.instance; litPrim = h.prim; litT = h.t; litU = h.u; litV = h.v; }      // the surface, unless a later layer contributes
            if (st.flags & RT64_GI_SAMPLE_COVERED) break;
        }
        const f3 rgb = st.rgb; const float rem = st.rem; const int lit = st.lit; const uint32_t layers = st.layers; uint32_t flags = st.flags;
        f3 position = mk3s(0.0f), normal = mk3s(0.0f), radiance = mk3s(0.0f);
        TraceCounts cnt; cnt.nodes = 0; cnt.tris = 0;
        if (lit >= 0) {
            LightPoint pt;
            {
                const uint32_t k0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)litInstance);
                if (__ballot(litInstance != k0) == 0ull) gi_point_of_layer(P, inst_view(P, k0), litPrim, litT, litU, litV, rayOrigin, rayDirection, pt);
                else gi_point_of_layer(P, inst_view(P, litInstance), litPrim, litT, litU, litV, rayOrigin, rayDirection, pt);
            }
            position = pt.position; normal = pt.normal;
            flags |= RT64_GI_SAMPLE_SURFACE;
            if (LIGHT) {
                const f3 specular = pt.specular;
                f3 direct = mk3s(0.0f);
                if (pt.mask == 0u) flags |= RT64_GI_SAMPLE_UNLIT;                             // shade.h:645
                else {
                    float total = 0.0f;
                    uint32_t sCount = 0u, l = 0u;
                    for (; l < P.lightCount && sCount < RT64_MAX_LIGHTS; l++) {                // shade.h:650-656
                        const RT64_LIGHT Ll = load_const(P.lights + l);                         // uniform index: scalar loads
                        if (!(pt.mask & Ll.groupBits)) continue;
                        const float li = light_intensity_simple(Ll, position, normal, pt.ignoreNormalFactor);
                        if (li > RT_EPSILON) { sInt[sCount * RT_LANES] = li; sIdx[sCount * RT_LANES] = (uint8_t)l; total += li; sCount++; }
                    }
                    if (l < P.lightCount) flags |= RT64_GI_SAMPLE_TRUNCATED;
                    if (sCount > 0u) {                                                          // maxLightCount = 1: one draw (shade.h:657-670)
                        uint32_t chosen = 0; float invProbability = 1.0f;
                        if (sCount != 1u) {
                            const float r = blue_noise(P, kx, ky, kf).x * total;                // slice frameCount + 0: the same for every sample and bounce of the key
                            float rInt = sInt[0];
                            while (chosen < sCount - 1u && r >= rInt) { chosen++; rInt += sInt[chosen * RT_LANES]; }
                            invProbability = s_div(total, sInt[chosen * RT_LANES]);
                        }
                        const uint32_t cIdx = sIdx[chosen * RT_LANES];
                        // shade.h:594-632
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
                        for (uint32_t n = maxSamples; n > 0u; n--) {
                            f3 samplePosition = lp;          // radius 0: the disc offsets are finite numbers times 0 (shade.h:605-608)
                            if (lightPointRadius != 0.0f || !(lightDirection.x == lightDirection.x)) {
                                const f3 bn = blue_noise(P, kx, ky, kf + n);
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
                        direct = direct + (term * lShadow) * invProbability;
                    }
                }
                const f3 directLight = direct + pt.selfLight;                                  // passes.hip: compute_lights_random(...) + selfLight
                f3 in3 = ambientBase + mk3(P.ambientNoGIColor[0], P.ambientNoGIColor[1], P.ambientNoGIColor[2]);
                if (incoming) { const float *q = incoming + i * incomingStride; in3 = mk3(load_global(q), load_global(q + 1), load_global(q + 2)); }
                const f3 indirectLight = ((rgb * (1.0f - rem)) * (in3 + directLight)) * P.giDiffuseStrength;
                radiance = indirectLight;
            }
        }
        if (LIGHT && valid) {                                                                  // Y7
            f3 resIndirect = ambientBase;
            if (lit >= 0) resIndirect = resIndirect + radiance;
            const f3 bgColor = sky_over_background_envmap(P, rayDirection);
            radiance = resIndirect + bgColor * (P.giSkyStrength * rem);
        }
        keep_counts(P, cnt);
        u32x4 o0, o1, o2, o3;
        o0.x = __float_as_uint(radiance.x); o0.y = __float_as_uint(radiance.y); o0.z = __float_as_uint(radiance.z); o0.w = __float_as_uint(valid ? rem : 0.0f);
        o1.x = __float_as_uint(position.x); o1.y = __float_as_uint(position.y); o1.z = __float_as_uint(position.z); o1.w = flags;
        o2.x = __float_as_uint(normal.x); o2.y = __float_as_uint(normal.y); o2.z = __float_as_uint(normal.z); o2.w = lit >= 0 ? litInstance : 0xFFFFFFFFu;
        o3.x = layers; o3.y = 0u; o3.z = cnt.nodes; o3.w = cnt.tris;
        GOut dst = QUERY_OUT(samples + i);
        dst[0] = o0; dst[1] = o1; dst[2] = o2; dst[3] = o3;
    }
}

// Y10: the point of a hit.  A miss or a bad hit is RT64_GI_POINT_NONE; nothing is read through an out-of-range index.
__global__ __launch_bounds__(RT_BLOCK) void gi_point_kernel(FrameParams Pv, const RT64_RAY *rays, const RT64_RAY_HIT *hits, const float *lods, RT64_GI_POINT *points, uint64_t count) {
    PRef P = *kernel_params(); (void)Pv;
    const uint64_t stride = query_stride();
    for (uint64_t i = query_first(); i < count; i += stride) {
        const QueryRay ray = load_ray(QUERY_IN(rays + i));
        const QueryHit h = load_hit(QUERY_IN(hits + i));
        const float lod = lods ? load_global(lods + i) : 0.0f;
        const f3 rayDirection = mk3(ray.d[0], ray.d[1], ray.d[2]);
        const uint32_t instance = h.instance, prim = h.prim;
        LightPoint pt;
        pt.position = pt.normal = pt.specular = pt.selfLight = mk3s(0.0f); pt.ignoreNormalFactor = pt.shadowRayBias = pt.specularExponent = 0.0f; pt.mask = 0u; pt.flags = 0u;
        bool real = false;
        if (instance < P.instanceCount) {               // (unsigned: a negative instance is past the end)
            const uint32_t k0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)instance);
            if (__ballot(instance != k0) == 0ull) {
                if (prim < load_const(&P.instances[k0].triCount)) { point_of_hit(P, inst_view(P, k0), prim, h.u, h.v, rayDirection, lod, pt); real = true; }
            }
            else if (prim < load_const(&P.instances[instance].triCount)) { point_of_hit(P, inst_view(P, instance), prim, h.u, h.v, rayDirection, lod, pt); real = true; }
        }
        u32x4 o0, o1;
        o0.x = __float_as_uint(pt.position.x); o0.y = __float_as_uint(pt.position.y); o0.z = __float_as_uint(pt.position.z); o0.w = real ? 0u : (uint32_t)RT64_GI_POINT_NONE;
        o1.x = __float_as_uint(pt.normal.x); o1.y = __float_as_uint(pt.normal.y); o1.z = __float_as_uint(pt.normal.z); o1.w = real ? instance : 0xFFFFFFFFu;
        GOut dst = QUERY_OUT(points + i);
        dst[0] = o0; dst[1] = o1;
    }
}

// Y8: sample s of point i is record s * count + i of `first` (its second bounce, if the chain sent one, the same record of `second`; the walks' counters the same record
// of the RT64_RAY_LAYERS arrays).  indirect_kernel's accumulation without history: historyLength counts up from 0.
__global__ __launch_bounds__(RT_BLOCK) void gi_accumulate_kernel(FrameParams Pv, const RT64_GI_POINT *points, const RT64_GI_SAMPLE *firstSamples, const RT64_GI_SAMPLE *secondSamples,
                                                                 const RT64_RAY_LAYERS *firstWalks, const RT64_RAY_LAYERS *secondWalks, uint32_t giSamples, RT64_POINT_INDIRECT *records, uint64_t count) {
    PRef P = *kernel_params(); (void)Pv;
    const uint64_t stride = query_stride();
    for (uint64_t i = query_first(); i < count; i += stride) {
        const GIn in = QUERY_IN(points + i);
        const u32x4 a = in[0], b = in[1];
        f3 newIndirect = mk3s(0.0f); float historyLength = 0.0f, m1 = 0.0f, m2 = 0.0f;
        uint32_t flags = 0u, instance = b.w, rays = 0u, nodes = 0u, tris = 0u;
        if (a.w & RT64_GI_POINT_NONE) instance = 0xFFFFFFFFu;                                  // Y1: no point
        else if (!gi_point_usable(a, b, 0u, 0u)) flags = RT64_INDIRECT_BAD_POINT;
        else if (giSamples == 0u) {                                                            // I1 (passes.hip: the store of `ambient`)
            newIndirect = mk3(P.ambientBaseColor[0], P.ambientBaseColor[1], P.ambientBaseColor[2]) + mk3(P.ambientNoGIColor[0], P.ambientNoGIColor[1], P.ambientNoGIColor[2]);
            flags = RT64_INDIRECT_VALID;
        }
        else {
            flags = RT64_INDIRECT_VALID;
            float sumL = 0.0f, sumL2 = 0.0f;
            for (uint32_t s = 0; s < giSamples; s++) {
                const uint64_t at = (uint64_t)s * count + i;
                const GIn rec = QUERY_IN(firstSamples + at);
                const u32x4 r0 = rec[0], r1 = rec[1], r3 = rec[3];
                const f3 resIndirect = mk3(__uint_as_float(r0.x), __uint_as_float(r0.y), __uint_as_float(r0.z));
                historyLength = fminf(historyLength + 1.0f, 64.0f);
                newIndirect = lerp3(newIndirect, resIndirect, s_rcp(historyLength));
                { const float l = 0.2126f * resIndirect.x + 0.7152f * resIndirect.y + 0.0722f * resIndirect.z; sumL += l; sumL2 += l * l; }
                if (r1.w & RT64_GI_SAMPLE_BAD_HIT) flags |= RT64_INDIRECT_BAD_HIT;
                if (r1.w & RT64_GI_SAMPLE_VALID) rays++;
                nodes += r3.z; tris += r3.w;
                if (firstWalks) { const u32x4 w = QUERY_IN(firstWalks + at)[0]; nodes += w.z; tris += w.w; }
                if (secondSamples) {
                    const GIn rec2 = QUERY_IN(secondSamples + at);
                    const u32x4 q1 = rec2[1], q3 = rec2[3];
                    if (q1.w & RT64_GI_SAMPLE_BAD_HIT) flags |= RT64_INDIRECT_BAD_HIT;
                    if (q1.w & RT64_GI_SAMPLE_VALID) rays++;
                    nodes += q3.z; tris += q3.w;
                    if (secondWalks) { const u32x4 w = QUERY_IN(secondWalks + at)[0]; nodes += w.z; tris += w.w; }
                }
            }
            const float nS = (float)giSamples, alphaM = fminf(nS / historyLength, 1.0f);
            m1 = lerpf(0.0f, sumL / nS, alphaM); m2 = lerpf(0.0f, sumL2 / nS, alphaM);
        }
        u32x4 o0, o1, o2;
        o0.x = __float_as_uint(newIndirect.x); o0.y = __float_as_uint(newIndirect.y); o0.z = __float_as_uint(newIndirect.z); o0.w = __float_as_uint(historyLength);
        o1.x = __float_as_uint(m1); o1.y = __float_as_uint(m2); o1.z = flags; o1.w = instance;
        o2.x = rays; o2.y = nodes; o2.z = tris; o2.w = 0u;
        GOut dst = QUERY_OUT(records + i);
        dst[0] = o0; dst[1] = o1; dst[2] = o2;
    }
}

}  // namespace

hipError_t launch_gi_rays(const FrameParams &P, const void *source, uint32_t strideWords, bool perRay, uint32_t needFlags, uint32_t refuseFlags, const void *keys, uint64_t first,
                          uint64_t points, uint32_t giSamples, uint32_t slotTop, bool second, void *rays, uint64_t count, hipStream_t s) {
    if (!count) return hipSuccess;
    hipLaunchKernelGGL(gi_ray_kernel, query_grid(count), dim3(RT_BLOCK), 0, s, P, static_cast<const u32x4 *>(source), strideWords, perRay ? 1u : 0u, needFlags, refuseFlags,
                       static_cast<const RT64_LIGHT_SAMPLE_KEY *>(keys), first, points, giSamples, slotTop, second ? 1u : 0u, static_cast<RT64_RAY *>(rays), count);
    return hipGetLastError();
}

hipError_t launch_gi_shade(const FrameParams &P, const void *rays, const void *hits, uint32_t maxLayers, const void *keys, uint64_t first, uint64_t points, const void *incoming,
                           uint32_t incomingStride, uint32_t diSamples, bool light, void *samples, uint64_t count, hipStream_t s) {
    if (!count) return hipSuccess;
    const RT64_RAY *r = static_cast<const RT64_RAY *>(rays); const RT64_RAY_HIT *h = static_cast<const RT64_RAY_HIT *>(hits);
    const RT64_LIGHT_SAMPLE_KEY *k = static_cast<const RT64_LIGHT_SAMPLE_KEY *>(keys); RT64_GI_SAMPLE *o = static_cast<RT64_GI_SAMPLE *>(samples);
    if (!light) {
        hipLaunchKernelGGL((gi_shade_kernel<false, false>), query_grid(count), dim3(RT_BLOCK), 0, s, P, r, h, k, first, points, static_cast<const float *>(nullptr), 0u, 0u, o, count, maxLayers);
        return hipGetLastError();
    }
    decltype(&gi_shade_kernel<true, false>) kernels[2] = { gi_shade_kernel<true, false>, gi_shade_kernel<true, true> };
    // the candidate columns behind the cache image: slots x RT_BLOCK floats, then slots x RT_BLOCK bytes
    const size_t slots = (P.lightCount < RT64_MAX_LIGHTS ? P.lightCount : (uint32_t)RT64_MAX_LIGHTS) + 1u, columns = slots * RT_BLOCK * (sizeof(float) + 1);
    return launch_cached(kernels, P, count, columns, s, r, h, k, first, points, static_cast<const float *>(incoming), incomingStride, diSamples, o, count, maxLayers);
}

hipError_t launch_gi_points(const FrameParams &P, const void *rays, const void *hits, const void *lods, void *points, uint64_t count, hipStream_t s) {
    if (!count) return hipSuccess;
    hipLaunchKernelGGL(gi_point_kernel, query_grid(count), dim3(RT_BLOCK), 0, s, P, static_cast<const RT64_RAY *>(rays), static_cast<const RT64_RAY_HIT *>(hits),
                       static_cast<const float *>(lods), static_cast<RT64_GI_POINT *>(points), count);
    return hipGetLastError();
}

hipError_t launch_gi_accumulate(const FrameParams &P, const void *points, const void *firstSamples, const void *secondSamples, const void *firstWalks, const void *secondWalks,
                                uint32_t giSamples, void *records, uint64_t count, hipStream_t s) {
    if (!count) return hipSuccess;
    hipLaunchKernelGGL(gi_accumulate_kernel, query_grid(count), dim3(RT_BLOCK), 0, s, P, static_cast<const RT64_GI_POINT *>(points), static_cast<const RT64_GI_SAMPLE *>(firstSamples),
                       static_cast<const RT64_GI_SAMPLE *>(secondSamples), static_cast<const RT64_RAY_LAYERS *>(firstWalks), static_cast<const RT64_RAY_LAYERS *>(secondWalks), giSamples,
                       static_cast<RT64_POINT_INDIRECT *>(records), count);
    return hipGetLastError();
}
