// query_common.h -- the scaffold every ray-query kernel shares (launch shape and launch lines, record loads and stores, the walk's prologue).  What the
// kernels that light a point share beyond it -- the shaded point, the light sample, the shadow walk -- is query_shading.h.
//
// Every query kernel runs one record per lane, RT_BLOCK threads per workgroup, at most RT_GRID_BLOCKS workgroups that stride over the records in the order given
// (no sorting: a caller that wants coherent waves hands coherent rays in neighbouring slots), with 16-byte loads and stores.
//   A walk kernel (rays -> hits) is its launch line (launch_walk, or launch_cached for a kernel with one template switch), fill_cache + lane_stack, load_ray + query_ray_valid, trace_ray of trace.h with its own hit handler,
//   and its record store (the macro STORE_QUERY_HIT for an RT64_RAY_HIT).  The walk runs from the LDS scene cache when the frame's table slot has a cache image,
//   otherwise the one-step-per-trip HBM walk with its LDS stack and the query's spill slab.
//   A resolve kernel (rays + hits -> records) is load_ray + load_hit, its own miss record and per-hit function, and its own record pack.  No LDS, no stack.  The
//   choice between a wave-uniform and a per-lane instance read stays written out in hit_surface_kernel and hit_material_kernel (surface.hip says why).
// What a new query kind supplies itself: the handler (or per-hit function), the record, and the rule both are held to.
#pragma once
#include "kernels.h"
#include "shade.h"

typedef const u32x4 __attribute__((address_space(1))) *GIn;
typedef u32x4 __attribute__((address_space(1))) *GOut;
// A record of the caller's arrays as 16-byte words.  Macros, not functions, and applied in the kernel itself: the address arithmetic compiles differently (operands
// swapped, another schedule behind them) when the array pointer, a kernel argument, reaches the cast through a function parameter.
#define QUERY_IN(p) reinterpret_cast<GIn>(reinterpret_cast<uintptr_t>(p))
#define QUERY_OUT(p) reinterpret_cast<GOut>(reinterpret_cast<uintptr_t>(p))

DEV uint64_t query_first() { return (uint64_t)blockIdx.x * RT_BLOCK + threadIdx.x; }          // for (uint64_t i = query_first(); i < count; i += query_stride())
DEV uint64_t query_stride() { return (uint64_t)gridDim.x * RT_BLOCK; }
static inline dim3 query_grid(uint64_t count) {
    const uint64_t blocks = (count + RT_BLOCK - 1) / RT_BLOCK;
    return dim3((unsigned)(blocks < RT_GRID_BLOCKS ? blocks : RT_GRID_BLOCKS));
}
// Launches the FIRST x CACHED instantiation of a walk kernel that `flags` and the frame's cache image select: kernels[first][cached]; `args` are the kernel's between P and count.
template <class K, class... A> hipError_t launch_walk(K (&kernels)[2][2], const FrameParams &P, uint64_t count, uint32_t flags, hipStream_t s, A... args) {
    if (!count) return hipSuccess;
    const uint32_t cull = (flags & RT64_RAY_FLAG_CULL_BACK_FACING) ? 1u : 0u;
    const bool first = (flags & RT64_RAY_FLAG_ACCEPT_FIRST_HIT) != 0, cached = P.cacheWords != 0;
    hipLaunchKernelGGL(kernels[first][cached], query_grid(count), dim3(RT_BLOCK), (size_t)P.cacheWords * 16, s, P, args..., count, cull);
    return hipGetLastError();
}
// Launches the CACHED instantiation the frame's cache image selects: kernels[cached]; `extraLds` are the kernel's own dynamic LDS bytes behind the cache image, `args` its arguments after P.
template <class K, class... A> hipError_t launch_cached(K (&kernels)[2], const FrameParams &P, uint64_t count, size_t extraLds, hipStream_t s, A... args) {
    if (!count) return hipSuccess;
    hipLaunchKernelGGL(kernels[P.cacheWords != 0], query_grid(count), dim3(RT_BLOCK), (size_t)P.cacheWords * 16 + extraLds, s, P, args...);
    return hipGetLastError();
}

struct QueryRay { float o[3], d[3], tmin, tmax; };          // origin + tMin, direction + tMax
struct QueryHit { float t, u, v; uint32_t instance, prim; };          // an RT64_RAY_HIT without its counters
DEV QueryRay load_ray(GIn ray) {
    const u32x4 a = ray[0], b = ray[1];
    return { { __uint_as_float(a.x), __uint_as_float(a.y), __uint_as_float(a.z) }, { __uint_as_float(b.x), __uint_as_float(b.y), __uint_as_float(b.z) },
             __uint_as_float(a.w), __uint_as_float(b.w) };
}
// Q6: NaN anywhere, inf in origin or direction, tMin >= tMax (false for a NaN too) or a zero direction: the ray is answered without a walk
DEV bool query_ray_valid(const float o[3], const float d[3], float tmin, float tmax) {
    bool ok = tmin < tmax && (d[0] != 0.0f || d[1] != 0.0f || d[2] != 0.0f);
#pragma unroll
    for (int k = 0; k < 3; k++) ok = ok && __builtin_isfinite(o[k]) && __builtin_isfinite(d[k]);
    return ok;
}

// ---- walk kernels ----------------------------------------------------------------------------------------------------------------------------------------------
// The __shared__ arrays stay declared in the kernel (ldsStack's size depends on CACHED).  CACHED: the frame's LDS scene cache image is copied in once per workgroup
// (fill_scene_cache of trace.h, the frame kernels' own) and the walk reads nodes and instance records from LDS.
#define QUERY_STACK_WORDS(CACHED) ((CACHED) ? RT_STACK_LDS_CACHED / 2 : RT_STACK_LDS)
template <bool CACHED> DEV void fill_cache(PRef P, u32x4_lds *dynLds) {      // every thread takes part before any of them leaves its ray loop
    if (CACHED) fill_scene_cache(P, dynLds);
}
// this lane's column in its wave's [entry][lane] block (wave64: a push / pop is one conflict-free ds access), and its slab in HBM.  A CACHED kernel then calls
// stk.use_cache(dynLds) itself: handed through here, the cache pointer changes the register allocation of ray_query_kernel<*, true>.
template <bool CACHED> DEV TraceStack lane_stack(PRef P, uint32_t *ldsStack) {
    TraceStack stk;
    uint32_t *block = ldsStack + (threadIdx.x >> 6) * QUERY_STACK_WORDS(CACHED) * RT_LANES;
    stk.lds = (LdsU32Ptr)(block + (threadIdx.x & 63u));
    stk.lds16 = (LdsI16Ptr)block + (threadIdx.x & 63u);
    stk.spill = (GlobalU32Ptr)(P.traversalStack + ((size_t)blockIdx.x * RT_BLOCK + threadIdx.x) * (RT_STACK_SPILL_HEADER + RT_STACK_SPILL) + RT_STACK_SPILL_HEADER);
    stk.cache = nullptr; stk.ldsEntries = RT_STACK_LDS;
    return stk;
}
DEV void keep_counts(PRef P, TraceCounts &cnt) { if (!P.countTraversal) { cnt.nodes = 0; cnt.tris = 0; } }
// Stores an RT64_RAY_HIT from its five fields and the walk's counters.  A macro: through a function ray_query_kernel<true, *> materialises three constants in another order.
#define STORE_QUERY_HIT(hit, t, u, v, instance, prim, cnt) do { \
        u32x4 r0_, r1_; \
        r0_.x = __float_as_uint(t); r0_.y = __float_as_uint(u); r0_.z = __float_as_uint(v); r0_.w = (instance); \
        r1_.x = (prim); r1_.y = (cnt).nodes; r1_.z = (cnt).tris; r1_.w = 0u; \
        GOut dst_ = QUERY_OUT(hit); dst_[0] = r0_; dst_[1] = r1_; \
    } while (0)

// ---- resolve kernels -------------------------------------------------------------------------------------------------------------------------------------------
DEV QueryHit load_hit(GIn hit) {          // t, u, v, instance / primitive, counters
    const u32x4 h0 = hit[0], h1 = hit[1];
    return { __uint_as_float(h0.x), __uint_as_float(h0.y), __uint_as_float(h0.z), h0.w, h1.x };
}
