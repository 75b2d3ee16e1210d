// query.hip -- batched ray queries against the scene of a view's last frame (RT64_TraceViewRays, include/rt64_query.h; rules Q1-Q7 in DESIGN.md 4).
//
// One ray per lane, RT_BLOCK threads per workgroup, at most RT_GRID_BLOCKS workgroups that stride over the rays in the order given (no sorting: a
// caller that wants coherent waves hands coherent rays in neighbouring slots).  The walk is trace_ray of trace.h -- R1-R5, the same device functions
// the frame's rays run -- from the LDS scene cache when the frame's table slot has a cache image, otherwise the one-step-per-trip HBM walk with its
// LDS stack and the query's own spill slab.  The hit handler is DXR FORCE_OPAQUE: every intersection commits (Q2), or ends the walk (Q3).
#include "kernels.h"
#include "trace.h"

namespace {

struct QueryHit { float t, u, v; uint32_t instance, prim; };

// Q6: NaN anywhere, inf in origin or direction, tMin >= tMax (false for a NaN too) or a zero direction: the ray misses without a walk
DEV bool query_ray_valid(const float o[3], const float d[3], float tmin, float tmax) {
    bool ok = tmin < tmax && (d[0] != 0.0f || d[1] != 0.0f || d[2] != 0.0f);
#pragma unroll
    for (int k = 0; k < 3; k++) ok = ok && __builtin_isfinite(o[k]) && __builtin_isfinite(d[k]);
    return ok;
}

// FIRST: the walk ends at the first intersection (Q3); otherwise every intersection commits tmax = t (Q2).
// CACHED: the frame's LDS scene cache image is copied in once per workgroup and the walk reads nodes and instance records from LDS.
template <bool FIRST, bool CACHED>
__global__ __launch_bounds__(RT_BLOCK) void ray_query_kernel(FrameParams Pv, const RT64_RAY *rays, RT64_RAY_HIT *hits, uint64_t count, uint32_t cullBackFaces) {
    PRef P = *kernel_params(); (void)Pv;
    constexpr uint32_t STACK_WORDS = CACHED ? RT_STACK_LDS_CACHED / 2 : RT_STACK_LDS;
    __shared__ uint32_t ldsStack[STACK_WORDS * RT_BLOCK];
    extern __shared__ u32x4_lds dynLds[];
    if (CACHED) {         // every thread takes part before any of them leaves the loop below
        typedef const u32x4 __attribute__((address_space(1))) *G4;
        G4 src = reinterpret_cast<G4>(reinterpret_cast<uintptr_t>(P.cacheImage));
        for (uint32_t t = threadIdx.x; t < P.cacheWords; t += RT_BLOCK) dynLds[t] = src[t];
        __syncthreads();
    }
    TraceStack stk;
    {   // this lane's column in its wave's [entry][lane] block (wave64: a push / pop is one conflict-free ds access), and its slab in HBM
        uint32_t *block = ldsStack + (threadIdx.x >> 6) * STACK_WORDS * RT_LANES;
        stk.lds = (LdsU32Ptr)(block + (threadIdx.x & 63u));
        stk.lds16 = (LdsI16Ptr)block + (threadIdx.x & 63u);
        stk.spill = (GlobalU32Ptr)(P.traversalStack + ((size_t)blockIdx.x * RT_BLOCK + threadIdx.x) * (RT_STACK_SPILL_HEADER + RT_STACK_SPILL) + RT_STACK_SPILL_HEADER);
        stk.cache = nullptr; stk.ldsEntries = RT_STACK_LDS;
        if (CACHED) stk.use_cache(dynLds);
    }
    typedef const u32x4 __attribute__((address_space(1))) *GIn;
    typedef u32x4 __attribute__((address_space(1))) *GOut;
    const uint64_t stride = (uint64_t)gridDim.x * RT_BLOCK;
    for (uint64_t i = (uint64_t)blockIdx.x * RT_BLOCK + threadIdx.x; i < count; i += stride) {
        GIn src = reinterpret_cast<GIn>(reinterpret_cast<uintptr_t>(rays + i));
        const u32x4 a = src[0], b = src[1];          // origin + tMin, direction + tMax
        const float o[3] = { __uint_as_float(a.x), __uint_as_float(a.y), __uint_as_float(a.z) };
        const float d[3] = { __uint_as_float(b.x), __uint_as_float(b.y), __uint_as_float(b.z) };
        const float tmin = __uint_as_float(a.w), tmax = __uint_as_float(b.w);
        QueryHit h; h.t = INFINITY; h.u = 0.0f; h.v = 0.0f; h.instance = 0xFFFFFFFFu; h.prim = 0xFFFFFFFFu;
        TraceCounts cnt; cnt.nodes = 0; cnt.tris = 0;
        if (query_ray_valid(o, d, tmin, tmax))
            trace_ray<CACHED>(P, o, d, tmin, tmax, cullBackFaces != 0, stk,
                              [&](float t, float u, float v, uint32_t instance, uint32_t prim, float &tm, uint32_t, float) -> bool {
                                  h.t = t; h.u = u; h.v = v; h.instance = instance; h.prim = prim;
                                  tm = t;
                                  return FIRST;
                              }, cnt);
        if (!P.countTraversal) { cnt.nodes = 0; cnt.tris = 0; }
        u32x4 r0, r1;
        r0.x = __float_as_uint(h.t); r0.y = __float_as_uint(h.u); r0.z = __float_as_uint(h.v); r0.w = h.instance;
        r1.x = h.prim; r1.y = cnt.nodes; r1.z = cnt.tris; r1.w = 0u;
        GOut dst = reinterpret_cast<GOut>(reinterpret_cast<uintptr_t>(hits + i));
        dst[0] = r0; dst[1] = r1;
    }
}

}  // namespace

size_t ray_query_spill_bytes() {
    return (size_t)RT_GRID_BLOCKS * RT_BLOCK * (RT_STACK_SPILL_HEADER + RT_STACK_SPILL) * sizeof(uint32_t);
}

hipError_t launch_ray_query(const FrameParams &P, const void *rays, void *hits, uint64_t count, uint32_t flags, hipStream_t s) {
    if (!count) return hipSuccess;
    const uint64_t blocks = (count + RT_BLOCK - 1) / RT_BLOCK;
    const dim3 grid((unsigned)(blocks < RT_GRID_BLOCKS ? blocks : RT_GRID_BLOCKS)), block(RT_BLOCK);
    const RT64_RAY *r = static_cast<const RT64_RAY *>(rays); RT64_RAY_HIT *h = static_cast<RT64_RAY_HIT *>(hits);
    const uint32_t cull = (flags & RT64_RAY_FLAG_CULL_BACK_FACING) ? 1u : 0u;
    const size_t lds = (size_t)P.cacheWords * 16;
    const bool first = (flags & RT64_RAY_FLAG_ACCEPT_FIRST_HIT) != 0;
    if (P.cacheWords && first) hipLaunchKernelGGL((ray_query_kernel<true, true>), grid, block, lds, s, P, r, h, count, cull);
    else if (P.cacheWords) hipLaunchKernelGGL((ray_query_kernel<false, true>), grid, block, lds, s, P, r, h, count, cull);
    else if (first) hipLaunchKernelGGL((ray_query_kernel<true, false>), grid, block, 0, s, P, r, h, count, cull);
    else hipLaunchKernelGGL((ray_query_kernel<false, false>), grid, block, 0, s, P, r, h, count, cull);
    return hipGetLastError();
}
