// query.hip -- batched ray queries against the scene of a view's last frame (RT64_TraceViewRays, include/rt64_query.h; rules Q1-Q7 in DESIGN.md 4).
//
// The plain walk kernel of query_common.h: the walk is trace_ray of trace.h -- R1-R5, the same device functions the frame's rays run -- and the hit handler is
// DXR FORCE_OPAQUE: every intersection commits (Q2), or ends the walk (Q3).
#include "query_common.h"

namespace {

// FIRST: the walk ends at the first intersection (Q3); otherwise every intersection commits tmax = t (Q2).
template <bool FIRST, bool CACHED>
__global__ __launch_bounds__(RT_BLOCK) void ray_query_kernel(FrameParams Pv, const RT64_RAY *rays, RT64_RAY_HIT *hits, uint64_t count, uint32_t cullBackFaces) {
    PRef P = *kernel_params(); (void)Pv;
    __shared__ uint32_t ldsStack[QUERY_STACK_WORDS(CACHED) * RT_BLOCK];
    extern __shared__ u32x4_lds dynLds[];
    fill_cache<CACHED>(P, dynLds);
    TraceStack stk = lane_stack<CACHED>(P, ldsStack);
    if (CACHED) stk.use_cache(dynLds);
    const uint64_t stride = query_stride();
    for (uint64_t i = query_first(); i < count; i += stride) {
        const QueryRay ray = load_ray(QUERY_IN(rays + i));
        QueryHit h; h.t = INFINITY; h.u = 0.0f; h.v = 0.0f; h.instance = 0xFFFFFFFFu; h.prim = 0xFFFFFFFFu;
        TraceCounts cnt; cnt.nodes = 0; cnt.tris = 0;
        if (query_ray_valid(ray.o, ray.d, ray.tmin, ray.tmax))
            trace_ray<CACHED>(P, ray.o, ray.d, ray.tmin, ray.tmax, cullBackFaces != 0, stk,
                              [&](float t, float u, float v, uint32_t instance, uint32_t prim, float &tm, uint32_t, float) -> bool {
                                  h.t = t; h.u = u; h.v = v; h.instance = instance; h.prim = prim;
                                  tm = t;
                                  return FIRST;
                              }, cnt);
        keep_counts(P, cnt);
        STORE_QUERY_HIT(hits + i, h.t, h.u, h.v, h.instance, h.prim, cnt);
    }
}

}  // namespace

size_t ray_query_spill_bytes() {
    return (size_t)RT_GRID_BLOCKS * RT_BLOCK * (RT_STACK_SPILL_HEADER + RT_STACK_SPILL) * sizeof(uint32_t);
}

hipError_t launch_ray_query(const FrameParams &P, const void *rays, void *hits, uint64_t count, uint32_t flags, hipStream_t s) {
    decltype(&ray_query_kernel<false, false>) kernels[2][2] = { { ray_query_kernel<false, false>, ray_query_kernel<false, true> }, { ray_query_kernel<true, false>, ray_query_kernel<true, true> } };
    return launch_walk(kernels, P, count, flags, s, static_cast<const RT64_RAY *>(rays), static_cast<RT64_RAY_HIT *>(hits));
}
