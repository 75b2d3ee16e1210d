// alpha_query.hip -- ray queries whose walk honours alpha (RT64_TraceViewRaysAlpha, RT64_TraceViewRayVisibility, include/rt64_alpha.h; rules K1-K10 in DESIGN.md 4).
//
// The launch shape is ray_query_kernel's (query.hip): one ray per lane, RT_BLOCK threads per workgroup, at most RT_GRID_BLOCKS workgroups that stride over the
// rays in the order given, 16-byte loads and stores, the walk trace_ray of trace.h from the LDS scene cache or from HBM with the query's spill slab.  What differs
// is the hit handler: an any-hit program that asks alpha.h for the alpha of the candidate.
//   alpha_query_kernel       closest hit among the intersections RT64_ShadeViewRayHits would not flag RT64_MATERIAL_CUTOUT (K2); a cutout neither commits nor
//                            shortens the ray.  Only a texture-edge instance runs the any-hit: one byte of its combiner, read per candidate, says so.
//   visibility_query_kernel  trace_shadow (shade.h) without a pixel: 1 minus the shadow alphas of every intersection in the window, 0 at a shadow-opaque instance (K5-K7).
//
// The instance differs per lane and steers control flow.  The any-hit is reached only by the lanes that hold a candidate in this trip of the walk, on an instance that
// needs it.  The closest-hit handler gathers its lane's instance record with vector loads (inst_view with a per-lane index, material.hip's form for mixed waves).  The
// frame's `waterfall` (one scalar pass per distinct instance) was built first: it held 2-6 more VGPRs, and on scenes with texture-edge shaders it ignored accepted
// candidates on about 2 % of the rays, so it does not ship here.  That is an OPEN DEFECT, not a settled choice: the cause is not explained (DESIGN.md 4 lists what was
// ruled out), and the visibility handler below -- trace_shadow's own, waterfall included, in a handler that may return false -- is the same construct; it passes its rule
// on all eight cases, which is evidence, not an explanation.
#include "kernels.h"
#include "alpha.h"

namespace {

// Q6: NaN anywhere, inf in origin or direction, tMin >= tMax (false for a NaN too) or a zero direction: the ray is answered without a walk
DEV bool alpha_ray_valid(const float o[3], const float d[3], float tmin, float tmax) {
    bool ok = tmin < tmax && (d[0] != 0.0f || d[1] != 0.0f || d[2] != 0.0f);
#pragma unroll
    for (int k = 0; k < 3; k++) ok = ok && __builtin_isfinite(o[k]) && __builtin_isfinite(d[k]);
    return ok;
}

// this lane's column in its wave's [entry][lane] block (wave64: a push / pop is one conflict-free ds access), and its slab in HBM
template <bool CACHED> DEV void lane_stack(PRef P, uint32_t *ldsStack, uint32_t stackWords, const u32x4_lds *cache, TraceStack &stk) {
    uint32_t *block = ldsStack + (threadIdx.x >> 6) * stackWords * RT_LANES;
    stk.lds = (LdsU32Ptr)(block + (threadIdx.x & 63u));
    stk.lds16 = (LdsI16Ptr)block + (threadIdx.x & 63u);
    stk.spill = (GlobalU32Ptr)(P.traversalStack + ((size_t)blockIdx.x * RT_BLOCK + threadIdx.x) * (RT_STACK_SPILL_HEADER + RT_STACK_SPILL) + RT_STACK_SPILL_HEADER);
    stk.cache = nullptr; stk.ldsEntries = RT_STACK_LDS;
    if (CACHED) stk.use_cache(cache);
}

template <bool CACHED> DEV void fill_cache(PRef P, u32x4_lds *dynLds) {      // every thread takes part before any of them leaves its ray loop
    if (!CACHED) return;
    typedef const u32x4 __attribute__((address_space(1))) *G4;
    G4 src = reinterpret_cast<G4>(reinterpret_cast<uintptr_t>(P.cacheImage));
    for (uint32_t t = threadIdx.x; t < P.cacheWords; t += RT_BLOCK) dynLds[t] = src[t];
    __syncthreads();
}

typedef const u32x4 __attribute__((address_space(1))) *GIn;
typedef u32x4 __attribute__((address_space(1))) *GOut;

// FIRST: the walk ends at the first intersection K2 accepts (K3); otherwise every accepted intersection commits tmax = t.
template <bool FIRST, bool CACHED>
__global__ __launch_bounds__(RT_BLOCK) void alpha_query_kernel(FrameParams Pv, const RT64_RAY *rays, const float *lods, RT64_RAY_HIT *hits, uint64_t count, uint32_t cullBackFaces) {
    PRef P = *kernel_params(); (void)Pv;
    constexpr uint32_t STACK_WORDS = CACHED ? RT_STACK_LDS_CACHED / 2 : RT_STACK_LDS;
    __shared__ uint32_t ldsStack[STACK_WORDS * RT_BLOCK];
    extern __shared__ u32x4_lds dynLds[];
    fill_cache<CACHED>(P, dynLds);
    TraceStack stk;
    lane_stack<CACHED>(P, ldsStack, STACK_WORDS, dynLds, stk);
    const uint64_t stride = (uint64_t)gridDim.x * RT_BLOCK;
    for (uint64_t i = (uint64_t)blockIdx.x * RT_BLOCK + threadIdx.x; i < count; i += stride) {
        GIn src = reinterpret_cast<GIn>(reinterpret_cast<uintptr_t>(rays + i));
        const u32x4 a = src[0], b = src[1];          // origin + tMin, direction + tMax
        const float o[3] = { __uint_as_float(a.x), __uint_as_float(a.y), __uint_as_float(a.z) };
        const float d[3] = { __uint_as_float(b.x), __uint_as_float(b.y), __uint_as_float(b.z) };
        const float tmin = __uint_as_float(a.w), tmax = __uint_as_float(b.w);
        const float lod = lods ? load_global(lods + i) : 0.0f;
        float ht = INFINITY, hu = 0.0f, hv = 0.0f; uint32_t hInstance = 0xFFFFFFFFu, hPrim = 0xFFFFFFFFu;
        TraceCounts cnt; cnt.nodes = 0; cnt.tris = 0;
        if (alpha_ray_valid(o, d, tmin, tmax))
            trace_ray<CACHED>(P, o, d, tmin, tmax, cullBackFaces != 0, stk,
                              [&](float t, float u, float v, uint32_t instance, uint32_t prim, float &tm, uint32_t, float) -> bool {
                                  if (load_global(&P.instances[instance].cc.optTextureEdge)) {      // K2: every other instance commits as in Q2
                                      const float alpha = surface_alpha_at_lod(P, inst_view(P, instance), prim, u, v, lod);
                                      if (!(alpha > RT64_EDGE_ALPHA)) return false;          // H6: a cutout neither commits nor shortens the ray
                                  }
                                  ht = t; hu = u; hv = v; hInstance = instance; hPrim = prim;
                                  tm = t;
                                  return FIRST;
                              }, cnt);
        if (!P.countTraversal) { cnt.nodes = 0; cnt.tris = 0; }
        u32x4 r0, r1;
        r0.x = __float_as_uint(ht); r0.y = __float_as_uint(hu); r0.z = __float_as_uint(hv); r0.w = hInstance;
        r1.x = hPrim; r1.y = cnt.nodes; r1.z = cnt.tris; r1.w = 0u;
        GOut dst = reinterpret_cast<GOut>(reinterpret_cast<uintptr_t>(hits + i));
        dst[0] = r0; dst[1] = r1;
    }
}

template <bool CACHED>
__global__ __launch_bounds__(RT_BLOCK) void visibility_query_kernel(FrameParams Pv, const RT64_RAY *rays, RT64_RAY_VISIBILITY *out, uint64_t count, uint32_t cullBackFaces) {
    PRef P = *kernel_params(); (void)Pv;
    constexpr uint32_t STACK_WORDS = CACHED ? RT_STACK_LDS_CACHED / 2 : RT_STACK_LDS;
    __shared__ uint32_t ldsStack[STACK_WORDS * RT_BLOCK];
    extern __shared__ u32x4_lds dynLds[];
    fill_cache<CACHED>(P, dynLds);
    TraceStack stk;
    lane_stack<CACHED>(P, ldsStack, STACK_WORDS, dynLds, stk);
    const uint64_t stride = (uint64_t)gridDim.x * RT_BLOCK;
    for (uint64_t i = (uint64_t)blockIdx.x * RT_BLOCK + threadIdx.x; i < count; i += stride) {
        GIn src = reinterpret_cast<GIn>(reinterpret_cast<uintptr_t>(rays + i));
        const u32x4 a = src[0], b = src[1];
        const float o[3] = { __uint_as_float(a.x), __uint_as_float(a.y), __uint_as_float(a.z) };
        const float d[3] = { __uint_as_float(b.x), __uint_as_float(b.y), __uint_as_float(b.z) };
        const float tmin = __uint_as_float(a.w), tmax = __uint_as_float(b.w);
        float visibility = 1.0f; uint32_t flags = 0u;
        TraceCounts cnt; cnt.nodes = 0; cnt.tris = 0;
        if (alpha_ray_valid(o, d, tmin, tmax)) {
            trace_ray<CACHED>(P, o, d, tmin, tmax, cullBackFaces != 0, stk,
                              [&](float, float u, float v, uint32_t instance, uint32_t prim, float &, uint32_t instFlags, float) -> bool {
                                  if (instFlags & GPU_INST_SHADOW_OPAQUE) { visibility = 0.0f; return true; }      // K6
                                  float sa = 0.0f;
                                  waterfall(instance, [&](uint32_t k) { sa = shadow_alpha_before_noise(P, inst_view(P, k), prim, u, v); });
                                  if (sa < 0.0f) return false;
                                  visibility = fmaxf(visibility - sa, 0.0f);
                                  return !(visibility > 0.0f);
                              }, cnt);
            flags = RT64_VISIBILITY_VALID | (visibility > 0.0f ? 0u : (uint32_t)RT64_VISIBILITY_BLOCKED);
        }
        if (!P.countTraversal) { cnt.nodes = 0; cnt.tris = 0; }
        u32x4 r;
        r.x = __float_as_uint(visibility); r.y = flags; r.z = cnt.nodes; r.w = cnt.tris;
        GOut dst = reinterpret_cast<GOut>(reinterpret_cast<uintptr_t>(out + i));
        dst[0] = r;
    }
}

}  // namespace

hipError_t launch_alpha_query(const FrameParams &P, const void *rays, const void *lods, void *hits, uint64_t count, uint32_t flags, hipStream_t s) {
    if (!count) return hipSuccess;
    const uint64_t blocks = (count + RT_BLOCK - 1) / RT_BLOCK;
    const dim3 grid((unsigned)(blocks < RT_GRID_BLOCKS ? blocks : RT_GRID_BLOCKS)), block(RT_BLOCK);
    const RT64_RAY *r = static_cast<const RT64_RAY *>(rays); const float *l = static_cast<const float *>(lods); RT64_RAY_HIT *h = static_cast<RT64_RAY_HIT *>(hits);
    const uint32_t cull = (flags & RT64_RAY_FLAG_CULL_BACK_FACING) ? 1u : 0u;
    const size_t lds = (size_t)P.cacheWords * 16;
    const bool first = (flags & RT64_RAY_FLAG_ACCEPT_FIRST_HIT) != 0;
    if (P.cacheWords && first) hipLaunchKernelGGL((alpha_query_kernel<true, true>), grid, block, lds, s, P, r, l, h, count, cull);
    else if (P.cacheWords) hipLaunchKernelGGL((alpha_query_kernel<false, true>), grid, block, lds, s, P, r, l, h, count, cull);
    else if (first) hipLaunchKernelGGL((alpha_query_kernel<true, false>), grid, block, 0, s, P, r, l, h, count, cull);
    else hipLaunchKernelGGL((alpha_query_kernel<false, false>), grid, block, 0, s, P, r, l, h, count, cull);
    return hipGetLastError();
}

hipError_t launch_visibility_query(const FrameParams &P, const void *rays, void *visibility, uint64_t count, uint32_t flags, hipStream_t s) {
    if (!count) return hipSuccess;
    const uint64_t blocks = (count + RT_BLOCK - 1) / RT_BLOCK;
    const dim3 grid((unsigned)(blocks < RT_GRID_BLOCKS ? blocks : RT_GRID_BLOCKS)), block(RT_BLOCK);
    const RT64_RAY *r = static_cast<const RT64_RAY *>(rays); RT64_RAY_VISIBILITY *o = static_cast<RT64_RAY_VISIBILITY *>(visibility);
    const uint32_t cull = (flags & RT64_RAY_FLAG_CULL_BACK_FACING) ? 1u : 0u;
    if (P.cacheWords) hipLaunchKernelGGL((visibility_query_kernel<true>), grid, block, (size_t)P.cacheWords * 16, s, P, r, o, count, cull);
    else hipLaunchKernelGGL((visibility_query_kernel<false>), grid, block, 0, s, P, r, o, count, cull);
    return hipGetLastError();
}
