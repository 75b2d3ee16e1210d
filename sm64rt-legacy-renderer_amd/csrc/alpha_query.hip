// alpha_query.hip -- ray queries whose walk honours alpha (RT64_TraceViewRaysAlpha, RT64_TraceViewRayVisibility, include/rt64_alpha.h; rules K1-K10 in DESIGN.md 4).
//
// Two walk kernels of query_common.h (launch shape, prologue, ray load and hit store are the header's).  What is theirs is the hit handler: an any-hit program
// that asks alpha.h for the alpha of the candidate.
//   alpha_query_kernel       closest hit among the intersections RT64_ShadeViewRayHits would not flag RT64_MATERIAL_CUTOUT (K2); a cutout neither commits nor
//                            shortens the ray.  Only a texture-edge instance runs the any-hit: one byte of its combiner, read per candidate, says so.
//   visibility_query_kernel  trace_shadow (shade.h) without a pixel: 1 minus the shadow alphas of every intersection in the window, 0 at a shadow-opaque instance (K5-K7).
//                            The walk and its handler are shadow_visibility of query_shading.h, the one the lighting and radiance kernels call per light sample.
//
// The instance differs per lane and steers control flow.  The any-hit is reached only by the lanes that hold a candidate in this trip of the walk, on an instance that
// needs it.  The closest-hit handler gathers its lane's instance record with vector loads (inst_view with a per-lane index, material.hip's form for mixed waves).  The
// frame's `waterfall` (one scalar pass per distinct instance) was built first: it held 2-6 more VGPRs, and on scenes with texture-edge shaders it ignored accepted
// candidates on about 2 % of the rays, so it does not ship here.  That is an OPEN DEFECT, not a settled choice; the visibility handler is the same construct, and the
// paragraph on what is and is not known stands once, at shadow_visibility (query_shading.h).
#include "query_shading.h"

namespace {

// FIRST: the walk ends at the first intersection K2 accepts (K3); otherwise every accepted intersection commits tmax = t.
template <bool FIRST, bool CACHED>
__global__ __launch_bounds__(RT_BLOCK) void alpha_query_kernel(FrameParams Pv, const RT64_RAY *rays, const float *lods, RT64_RAY_HIT *hits, uint64_t count, uint32_t cullBackFaces) {
    PRef P = *kernel_params(); (void)Pv;
    __shared__ uint32_t ldsStack[QUERY_STACK_WORDS(CACHED) * RT_BLOCK];
    extern __shared__ u32x4_lds dynLds[];
    fill_cache<CACHED>(P, dynLds);
    TraceStack stk = lane_stack<CACHED>(P, ldsStack);
    if (CACHED) stk.use_cache(dynLds);
    const uint64_t stride = query_stride();
    for (uint64_t i = query_first(); i < count; i += stride) {
        const QueryRay ray = load_ray(QUERY_IN(rays + i));
        const float lod = lods ? load_global(lods + i) : 0.0f;
        float ht = INFINITY, hu = 0.0f, hv = 0.0f; uint32_t hInstance = 0xFFFFFFFFu, hPrim = 0xFFFFFFFFu;
        TraceCounts cnt; cnt.nodes = 0; cnt.tris = 0;
        if (query_ray_valid(ray.o, ray.d, ray.tmin, ray.tmax))
            trace_ray<CACHED>(P, ray.o, ray.d, ray.tmin, ray.tmax, cullBackFaces != 0, stk,
                              [&](float t, float u, float v, uint32_t instance, uint32_t prim, float &tm, uint32_t, float) -> bool {
                                  if (load_global(&P.instances[instance].cc.optTextureEdge)) {      // K2: every other instance commits as in Q2
                                      const float alpha = surface_alpha_at_lod(P, inst_view(P, instance), prim, u, v, lod);
                                      if (!(alpha > RT64_EDGE_ALPHA)) return false;          // H6: a cutout neither commits nor shortens the ray
                                  }
                                  ht = t; hu = u; hv = v; hInstance = instance; hPrim = prim;
                                  tm = t;
                                  return FIRST;
                              }, cnt);
        keep_counts(P, cnt);
        STORE_QUERY_HIT(hits + i, ht, hu, hv, hInstance, hPrim, cnt);
    }
}

template <bool CACHED>
__global__ __launch_bounds__(RT_BLOCK) void visibility_query_kernel(FrameParams Pv, const RT64_RAY *rays, RT64_RAY_VISIBILITY *out, uint64_t count, uint32_t cullBackFaces) {
    PRef P = *kernel_params(); (void)Pv;
    __shared__ uint32_t ldsStack[QUERY_STACK_WORDS(CACHED) * RT_BLOCK];
    extern __shared__ u32x4_lds dynLds[];
    fill_cache<CACHED>(P, dynLds);
    TraceStack stk = lane_stack<CACHED>(P, ldsStack);
    if (CACHED) stk.use_cache(dynLds);
    const uint64_t stride = query_stride();
    for (uint64_t i = query_first(); i < count; i += stride) {
        const QueryRay ray = load_ray(QUERY_IN(rays + i));
        TraceCounts cnt; cnt.nodes = 0; cnt.tris = 0;
        float visibility = 1.0f; uint32_t flags = 0u;
        if (query_ray_valid(ray.o, ray.d, ray.tmin, ray.tmax)) {
            visibility = shadow_visibility<CACHED>(P, mk3(ray.o[0], ray.o[1], ray.o[2]), mk3(ray.d[0], ray.d[1], ray.d[2]), ray.tmin, ray.tmax, cullBackFaces != 0, stk, cnt);      // K5-K7
            flags = RT64_VISIBILITY_VALID | (visibility > 0.0f ? 0u : (uint32_t)RT64_VISIBILITY_BLOCKED);
        }
        keep_counts(P, cnt);
        u32x4 r;
        r.x = __float_as_uint(visibility); r.y = flags; r.z = cnt.nodes; r.w = cnt.tris;
        QUERY_OUT(out + i)[0] = r;
    }
}

}  // namespace

hipError_t launch_alpha_query(const FrameParams &P, const void *rays, const void *lods, void *hits, uint64_t count, uint32_t flags, hipStream_t s) {
    decltype(&alpha_query_kernel<false, false>) kernels[2][2] = { { alpha_query_kernel<false, false>, alpha_query_kernel<false, true> }, { alpha_query_kernel<true, false>, alpha_query_kernel<true, true> } };
    return launch_walk(kernels, P, count, flags, s, static_cast<const RT64_RAY *>(rays), static_cast<const float *>(lods), static_cast<RT64_RAY_HIT *>(hits));
}

hipError_t launch_visibility_query(const FrameParams &P, const void *rays, void *visibility, uint64_t count, uint32_t flags, hipStream_t s) {
    decltype(&visibility_query_kernel<false>) kernels[2] = { visibility_query_kernel<false>, visibility_query_kernel<true> };
    const uint32_t cull = (flags & RT64_RAY_FLAG_CULL_BACK_FACING) ? 1u : 0u;
    return launch_cached(kernels, P, count, 0, s, static_cast<const RT64_RAY *>(rays), static_cast<RT64_RAY_VISIBILITY *>(visibility), count, cull);
}
