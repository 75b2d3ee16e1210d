// radiance.hip -- the colour a ray brings back, and the sky behind it (RT64_SkyViewRays, RT64_SkyViewPixels, RT64_ComposeViewRayRadiance, include/rt64_radiance.h;
// rules W1-W12 in DESIGN.md 4).
//
// Two kernels of query_common.h:
//   ray_sky_kernel<PIXELS>    a resolve kernel, no LDS: per record 32 bytes in (the ray, two 16-byte loads) or 8 (the pixel) or nothing (pixels = NULL: the index is
//                             the pixel, F1), then the frame's own sky functions of shade.h -- fake_envmap_uv / sample_sky_plane / sky_over_background_envmap for a ray
//                             (what reflection_kernel, refraction and bounce rays call), sky_plane_uv / sample_sky_2d / sky_over_background_2d for a pixel (what the
//                             primary resolve calls) -- and two 16-byte stores.  The functions are called, not restated; the second call of the sampler folds into the
//                             first (same arguments, -ffp-contract=off).
//   ray_radiance_kernel<SHADOWS, CACHED>  a resolve kernel that also walks, hit_light_kernel's shape: fill_cache / lane_stack / use_cache and the spill slab are the walk
//                             kernels'.  Per ray the loop of reflection_kernel (passes.hip, "for (uint32_t hit = 0; hit < nhits; hit++)") over records (l, i) at
//                             l count + i, so that neighbouring lanes read neighbouring records, with the list ends of layer_weight_kernel (T7); then the light at
//                             the lit layer and the composition of passes.hip's `rgb = rgb * (ambient + directLight); rgb = rgb + (bgColor * resColor.w + resTransparent)`.
//                             SHADOWS = false is RT64_RADIANCE_FLAG_UNSHADOWED: no walk, hence no stack, no scene cache and no LDS at all.
//                             Per-lane state: the running sums (surface, transparent, rem), the lit layer's index and its hit (instance, primitive, u, v): the
//                             LightPoint is built from those once, after the loop -- a layer behind it would only overwrite it.  No per-lane array is indexed by a
//                             run-time value (layers.hip's head comment on scratch).  The instance of a layer is read by material.hip's scheme: scalar loads for a
//                             wave whose lanes agree on it, per-lane inst_view otherwise.  The frame constants are read per loop trip (kernel_params_here, as the
//                             frame's tile loops do): carried across the trips, the scalar loads of the sky's, the fog's and the lights' parameters left a dead
//                             spill slot in the frame (profiles/radiance_kernel_identity.txt); the Makefile compiles this file without the SLP vectorizer.
// What is restated.  layer_colour is the colour half of material_of_hit (material.hip) up to H6, then the frame's UNORM8 store (shade.h, rec.color): the same
// calls in the same order, so its alpha is surface_alpha_at_lod's bit for bit (alpha.h says why) and `transmittance` is layer_weight_kernel's.  One function for
// both was built and not kept: hit_material_kernel measured 2-3 % slower on shuffled rays with it (profiles/query_shading_kernel_identity.txt).
// What is shared.  The shaded point, the light sample and the shadow walk are query_shading.h's (point_of_hit, light_sample, sample_visibility), the copy
// hit_light_kernel calls; the admission loop around them is that kernel's without the eye light, the `unshadowed` sum and the counters, and the point's `flags`
// are not read here (the compiler drops them).  tests/test_gpu_radiance_query.py holds the records to RT64_ShadeViewRayHits and RT64_LightViewRayHits (the
// composition identity).
#include "query_shading.h"
#include "../../include/rt64_radiance.h"

namespace {

template <bool PIXELS>
__global__ __launch_bounds__(RT_BLOCK) void ray_sky_kernel(FrameParams Pv, const void *in, uint32_t firstPixel, RT64_RAY_SKY *sky, uint64_t count) {
    PRef P = *kernel_params(); (void)Pv;
    const uint64_t stride = query_stride();
    const uint32_t width = (uint32_t)P.width;
    const uint32_t frameFlags = (P.skyPlaneTexIndex < 0 ? (uint32_t)RT64_SKY_NO_TEXTURE : 0u) | (P.background.texels ? (uint32_t)RT64_SKY_BACKGROUND : 0u);
    for (uint64_t i = query_first(); i < count; i += stride) {
        f3 color = mk3s(0.0f); float alpha = 0.0f; f2 uv; uv.x = uv.y = 0.0f; uint32_t flags = 0u;
        if (PIXELS) {
            const uint2 *pixels = static_cast<const uint2 *>(in);
            uint32_t px, py;
            if (pixels) { const uint2 p = pixels[i]; px = p.x; py = p.y; }
            else { const uint32_t n = firstPixel + (uint32_t)i; px = n % width; py = n / width; }          // F1 (the host refused more records than pixels)
            f2 screenUV; screenUV.x = ((float)px + P.pixelJitter[0]) / (float)P.width; screenUV.y = ((float)py + P.pixelJitter[1]) / (float)P.height;      // W2: passes.hip's own line
            uv = sky_plane_uv(P, screenUV);
            alpha = sample_sky_2d(P, screenUV).w;
            color = sky_over_background_2d(P, screenUV);
            flags = (uint32_t)RT64_SKY_VALID | frameFlags;
        }
        else {
            const QueryRay ray = load_ray(QUERY_IN(static_cast<const RT64_RAY *>(in) + i));
            if (query_ray_valid(ray.o, ray.d, ray.tmin, ray.tmax)) {          // W1
                const f3 d = mk3(ray.d[0], ray.d[1], ray.d[2]);
                uv = fake_envmap_uv(d, P.skyYawOffset);
                alpha = sample_sky_plane(P, d).w;
                color = sky_over_background_envmap(P, d);
                flags = (uint32_t)RT64_SKY_VALID | frameFlags;
            }
        }
        u32x4 o0, o1;
        o0.x = __float_as_uint(color.x); o0.y = __float_as_uint(color.y); o0.z = __float_as_uint(color.z); o0.w = __float_as_uint(alpha);
        o1.x = __float_as_uint(uv.x); o1.y = __float_as_uint(uv.y); o1.z = flags; o1.w = 0u;
        GOut dst = QUERY_OUT(sky + i);
        dst[0] = o0; dst[1] = o1;
    }
}

// W4 for one real hit of instance `in`: material_of_hit's colour (H4, H5, the mix, the multiplier, H6), then the frame's UNORM8 store
DEV f4 layer_colour(PRef P, const InstView &in, uint32_t prim, float u, float v, float lod) {
    const GpuCombiner &cc = in.cc;
    const RT64_MATERIAL &mat = in.material;
    const float b[3] = { 1.0f - u - v, u, v };
    const f4 mix = mk4(mat.diffuseColorMix.x, mat.diffuseColorMix.y, mat.diffuseColorMix.z, mat.diffuseColorMix.w);
    VertexData vd;
    get_vertex_data(in, prim, b, false, vd);
    f4 t0 = mk4(0, 0, 0, 0);
    const f4 t1 = mk4(1.0f, 0.0f, 1.0f, 1.0f);
    if (cc.useTex0) {                                                                       // H4
        float unused;
        const f4 tex = tex_sample_lod(tex_view(P.textures + in.texDiffuse), vd.vertexUV.x, vd.vertexUV.y, lod, in.filter, in.hAddr, in.vAddr, unused);
        const float k = fmaxf(-mix.w, 0.0f);
        t0 = mk4(lerpf(tex.x, mix.x, k), lerpf(tex.y, mix.y, k), lerpf(tex.z, mix.z, k), tex.w);
    }
    f4 result;                                                                              // H5
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
    if (cc.optTextureEdge && result.w > RT64_EDGE_ALPHA) result.w = 1.0f;                   // H6 (shade.h: `if (result.w > 0.3f) result.w = 1.0f`)
    return mk4(q_unorm8(result.x), q_unorm8(result.y), q_unorm8(result.z), q_unorm8(result.w));      // shade.h: rec.color
}

// The running sums of reflection_kernel's loop (W3)
struct RadianceState { f3 surface, transparent; float rem; int lit; uint32_t shaded, flags; };

// W4 and W5 for one real hit of instance `in`: the body of reflection_kernel's loop (passes.hip) without its Fresnel share
DEV void layer_step(PRef P, const InstView &in, const QueryHit &h, uint32_t l, f3 rayOrigin, f3 rayDirection, float lod, bool fogFromCamera, f3 ambient, RadianceState &s) {
    const RT64_MATERIAL &m = in.material;
    const f4 hitColor = layer_colour(P, in, h.prim, h.u, h.v, lod);
    float alphaContrib = s.rem * hitColor.w;
    if (alphaContrib >= RT_EPSILON) {
        const float dist = h.t - m.depthBias;                                             // shade.h: rec.dist
        const f3 vertexPosition = rayOrigin + rayDirection * (dist + m.depthBias);
        if (m.fogEnabled) {
            const f4 fog = fogFromCamera ? fog_from_camera(P, m, vertexPosition) : fog_from_origin(m, vertexPosition, rayOrigin);
            s.transparent = s.transparent + xyz(fog) * (fog.w * alphaContrib);
            alphaContrib *= (1.0f - fog.w);
            s.flags |= RT64_RADIANCE_FOGGED;
        }
        if (m.lightGroupMaskBits > 0) { s.surface.x += hitColor.x * alphaContrib; s.surface.y += hitColor.y * alphaContrib; s.surface.z += hitColor.z * alphaContrib; }
        else s.transparent = s.transparent + (xyz(hitColor) * alphaContrib) * (ambient + ld_v3(m.selfLight));
        s.lit = (int)l;                                                                   // every contributing layer, lit or not (passes.hip: resInstanceId)
        s.shaded++;
        s.rem *= (1.0f - hitColor.w);
    }
    if (s.rem <= RT_EPSILON) s.flags |= RT64_RADIANCE_COVERED;
}

// SHADOWS = false (RT64_RADIANCE_FLAG_UNSHADOWED): nothing is walked, so the kernel has no stack and no scene cache -- a resolve kernel like layer_weight_kernel
template <bool SHADOWS, bool CACHED>
__global__ __launch_bounds__(RT_BLOCK) void ray_radiance_kernel(FrameParams Pv, const RT64_RAY *rays, const RT64_RAY_HIT *hits, const float *lods, RT64_RAY_RADIANCE *radiance,
                                                                uint64_t count, uint32_t maxLayers, uint32_t fogFromCamera) {
    PRef P = *kernel_params(); (void)Pv;
    __shared__ uint32_t ldsStack[SHADOWS ? QUERY_STACK_WORDS(CACHED) * RT_BLOCK : 1];
    extern __shared__ u32x4_lds dynLds[];
    TraceStack stk;
    if (SHADOWS) {
        fill_cache<CACHED>(P, dynLds);
        stk = lane_stack<CACHED>(P, ldsStack);
        if (CACHED) stk.use_cache(dynLds);
    }
    const uint64_t stride = query_stride();
    for (uint64_t i = query_first(); i < count; i += stride) {
        PRef P = *kernel_params_here();      // this trip's view of the frame constants: the sky's, the fog's and the lights' scalar loads stay in the trip that needs them
        const f3 ambient = mk3(P.ambientBaseColor[0], P.ambientBaseColor[1], P.ambientBaseColor[2]) + mk3(P.ambientNoGIColor[0], P.ambientNoGIColor[1], P.ambientNoGIColor[2]);
        const QueryRay ray = load_ray(QUERY_IN(rays + i));
        const float lod = lods ? load_global(lods + i) : 0.0f;
        const bool valid = query_ray_valid(ray.o, ray.d, ray.tmin, ray.tmax);
        const f3 rayOrigin = mk3(ray.o[0], ray.o[1], ray.o[2]), rayDirection = mk3(ray.d[0], ray.d[1], ray.d[2]);          // as given
        RadianceState st;
        st.surface = st.transparent = mk3s(0.0f); st.rem = 1.0f; st.lit = -1; st.shaded = 0u; st.flags = valid ? (uint32_t)RT64_RADIANCE_VALID : 0u;
        uint32_t litInstance = 0u, litPrim = 0u; float litU = 0.0f, litV = 0.0f;
        const uint32_t listed = valid ? maxLayers : 0u;          // a Q6-invalid ray reads no hit
        for (uint32_t l = 0; l < listed; l++) {
            const QueryHit h = load_hit(QUERY_IN(hits + ((uint64_t)l * count + i)));
            if ((int32_t)h.instance < 0) break;                                             // the list's end
            bool real = false;
            if (h.instance < P.instanceCount) {
                const uint32_t k0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)h.instance);
                if (__ballot(h.instance != k0) == 0ull) {       // the lanes in here agree: k0 is wave-uniform, inst_view's loads are scalar and the combiner's branches uniform
                    if (h.prim < load_const(&P.instances[k0].triCount)) { layer_step(P, inst_view(P, k0), h, l, rayOrigin, rayDirection, lod, fogFromCamera != 0u, ambient, st); real = true; }
                }
                else if (h.prim < load_const(&P.instances[h.instance].triCount)) { layer_step(P, inst_view(P, h.instance), h, l, rayOrigin, rayDirection, lod, fogFromCamera != 0u, ambient, st); real = true; }
            }
            if (!real) { st.flags |= RT64_RADIANCE_BAD_HIT; break; }
            if (st.lit == (int)l) { litInstance = h.instance; litPrim = h.prim; litU = h.u; litV = h.v; }      // the hit the light is taken at, unless a later layer contributes
            if (st.flags & RT64_RADIANCE_COVERED) break;
        }
        const f3 surface = st.surface, transparent = st.transparent; const float rem = st.rem; const int lit = st.lit; const uint32_t shaded = st.shaded; uint32_t flags = st.flags;
        // W6: hit_light_kernel's loop at the lit layer
        f3 light = mk3s(0.0f);
        if (lit >= 0) {
            LightPoint pt;
            {
                const uint32_t k0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)litInstance);
                if (__ballot(litInstance != k0) == 0ull) point_of_hit(P, inst_view(P, k0), litPrim, litU, litV, rayDirection, lod, pt);
                else point_of_hit(P, inst_view(P, litInstance), litPrim, litU, litV, rayDirection, lod, pt);
            }
            const f3 position = pt.position, normal = pt.normal, specular = pt.specular;
            f3 direct = mk3s(0.0f);
            uint32_t admitted = 0u;
            TraceCounts cnt; cnt.nodes = 0; cnt.tris = 0;
            if (pt.mask != 0u) {                                                             // P4: shade.h, compute_lights_random's first line
                uint32_t k = 0;
                for (; k < P.lightCount && admitted < RT64_MAX_LIGHTS; k++) {
                    const RT64_LIGHT L = load_const(P.lights + k);                          // uniform index: scalar loads
                    if (!(pt.mask & L.groupBits)) continue;
                    if (!(light_intensity_simple(L, position, normal, pt.ignoreNormalFactor) > RT_EPSILON)) continue;
                    admitted++;
                    // P5
                    const LightSample ls = light_sample(position, ld_v3(L.position), normal, rayDirection, L, pt.ignoreNormalFactor, pt.specularExponent);
                    const f3 term = ld_v3(L.diffuseColor) * ls.lambert + ld_v3(L.specularColor) * (specular * ls.sp);
                    const float visibility = SHADOWS ? sample_visibility<CACHED>(P, pt, ls, L, stk, cnt) : 1.0f;          // P6
                    direct = direct + term * visibility;
                }
                if (k < P.lightCount) flags |= RT64_RADIANCE_TRUNCATED;
            }
            light = ambient + (direct + pt.selfLight);                                       // passes.hip: ambient + (compute_lights_random(...) + selfLight)
            flags |= RT64_RADIANCE_LIT;
        }
        // W7
        f3 rgb = surface;
        if (lit >= 0) rgb = rgb * light;
        if (valid) {
            const f3 bgColor = sky_over_background_envmap(P, rayDirection);
            rgb = rgb + (bgColor * rem + transparent);
        }
        u32x4 o0, o1, o2, o3;
        o0.x = __float_as_uint(rgb.x); o0.y = __float_as_uint(rgb.y); o0.z = __float_as_uint(rgb.z); o0.w = flags;
        o1.x = __float_as_uint(surface.x); o1.y = __float_as_uint(surface.y); o1.z = __float_as_uint(surface.z); o1.w = __float_as_uint(rem);
        o2.x = __float_as_uint(transparent.x); o2.y = __float_as_uint(transparent.y); o2.z = __float_as_uint(transparent.z); o2.w = (uint32_t)lit;
        o3.x = __float_as_uint(light.x); o3.y = __float_as_uint(light.y); o3.z = __float_as_uint(light.z); o3.w = shaded;
        GOut dst = QUERY_OUT(radiance + i);
        dst[0] = o0; dst[1] = o1; dst[2] = o2; dst[3] = o3;
    }
}

}  // namespace

hipError_t launch_ray_sky(const FrameParams &P, const void *rays, void *sky, uint64_t count, hipStream_t s) {
    if (!count) return hipSuccess;
    hipLaunchKernelGGL(ray_sky_kernel<false>, query_grid(count), dim3(RT_BLOCK), 0, s, P, rays, 0u, static_cast<RT64_RAY_SKY *>(sky), count);
    return hipGetLastError();
}

hipError_t launch_pixel_sky(const FrameParams &P, const void *pixels, uint64_t firstPixel, void *sky, uint64_t count, hipStream_t s) {
    if (!count) return hipSuccess;
    hipLaunchKernelGGL(ray_sky_kernel<true>, query_grid(count), dim3(RT_BLOCK), 0, s, P, pixels, (uint32_t)firstPixel, static_cast<RT64_RAY_SKY *>(sky), count);
    return hipGetLastError();
}

hipError_t launch_ray_radiance(const FrameParams &P, const void *rays, const void *hits, const void *lods, void *radiance, uint64_t count, uint32_t maxLayers, uint32_t flags, hipStream_t s) {
    if (!count) return hipSuccess;
    const RT64_RAY *r = static_cast<const RT64_RAY *>(rays); const RT64_RAY_HIT *h = static_cast<const RT64_RAY_HIT *>(hits);
    const float *l = static_cast<const float *>(lods); RT64_RAY_RADIANCE *o = static_cast<RT64_RAY_RADIANCE *>(radiance);
    const uint32_t fogFromCamera = (flags & RT64_RADIANCE_FLAG_FOG_FROM_CAMERA) ? 1u : 0u;
    if (flags & RT64_RADIANCE_FLAG_UNSHADOWED) {
        hipLaunchKernelGGL((ray_radiance_kernel<false, false>), query_grid(count), dim3(RT_BLOCK), 0, s, P, r, h, l, o, count, maxLayers, fogFromCamera);
        return hipGetLastError();
    }
    decltype(&ray_radiance_kernel<true, false>) kernels[2] = { ray_radiance_kernel<true, false>, ray_radiance_kernel<true, true> };
    return launch_cached(kernels, P, count, 0, s, r, h, l, o, count, maxLayers, fogFromCamera);
}
