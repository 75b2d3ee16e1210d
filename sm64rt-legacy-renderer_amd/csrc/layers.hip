// layers.hip -- a ray's sorted hit list as a frame keeps it, and the weight of each of its layers in the frame's resolve (RT64_TraceViewRayLayers,
// RT64_WeighViewRayLayers, include/rt64_layers.h; rules T1-T12 in DESIGN.md 4).
//
// Two kernels of query_common.h:
//   layer_walk_kernel    a walk kernel.  fill_cache / lane_stack / use_cache are alpha_query_kernel's, and so is the head of its handler: K2's per-lane gather (alpha_query.hip's
//                        head comment has the open defect of `waterfall`).  Behind it stands the insertion of trace_surface<true> (pass_common.h:126-144), statement for
//                        statement -- the same comparisons in the same order, the same two places that lower tmax -- over another store:
//                          keys   16 floats per lane in LDS, [wave][entry][lane]: the insertion compares and shifts these alone (ds_read_b32 / ds_write_b32, conflict-free);
//                          slots  16 bytes per lane in LDS, the same layout: entry -> payload slot in bits 0-3, the instance's GPU_INST_OPAQUE in bit 7; shifted with the keys;
//                          slab   t, u, v, instance (16 bytes) and the primitive (4 bytes) of an entry, written ONCE to payload slot `slot` of this lane in HBM,
//                                 [workgroup][slot][thread], and never moved.  A full list hands the slot of the entry that leaves it (the frame's scratch slot 16) to the newcomer.
//                        The frame shifts 24 bytes per displaced slot through HBM on every insertion; here an insertion that displaces k entries costs k LDS
//                        reads and writes of 5 bytes and one 20-byte store.  After the walk the lane scans its slot bytes for the first opaque entry (T3), then the
//                        workgroup goes layer by layer: a lane gathers its entry from the slab and stores the record, or stores the miss record, neighbouring lanes to
//                        neighbouring records (16-byte stores, layer-major).
//                        LDS per workgroup of 256: 16 KB keys + 4 KB slots = 20 KB, next to the stack (8 KB with the scene cache, 24 KB without) and the cache (at most
//                        24 KB): 52 KB or 44 KB, three workgroups per CU of 160 KB.  No per-lane array is indexed by a run-time slot: such an array would live in scratch.
//   layer_weight_kernel  a resolve kernel, no LDS, no stack: per ray the loop of passes.hip:113-175 without its fog, Fresnel and light terms (T7), over records
//                        (l, i) at l count + i, so that neighbouring lanes read neighbouring records; alpha is surface_alpha_at_lod of alpha.h, then H6 and the
//                        frame's UNORM8 store.  A ray whose resolve has ended still stores its zeros.
#include "query_common.h"
#include "alpha.h"

namespace {

typedef float __attribute__((address_space(3))) *LdsF32Ptr;
typedef uint8_t __attribute__((address_space(3))) *LdsU8Ptr;
typedef u32x4 __attribute__((address_space(1))) *SlabU4Ptr;
typedef uint32_t __attribute__((address_space(1))) *SlabU32Ptr;

#define LAYER_OPAQUE_BIT 0x80u          // bit 7 of a slot byte: the entry's instance is O1-opaque

// payload slab: [RT_GRID_BLOCKS][16][RT_BLOCK] 16-byte words (t, u, v, instance), then as many uint32 (primitive)
constexpr size_t LAYER_SLAB_ENTRIES = (size_t)RT_GRID_BLOCKS * RT64_RAY_LAYERS_MAX * RT_BLOCK;

template <bool CACHED>
__global__ __launch_bounds__(RT_BLOCK) void layer_walk_kernel(FrameParams Pv, const RT64_RAY *rays, const float *lods, RT64_RAY_HIT *hits, RT64_RAY_LAYERS *layers, u32x4 *slab,
                                                              uint64_t count, uint32_t maxLayers, uint32_t cullBackFaces) {
    PRef P = *kernel_params(); (void)Pv;
    __shared__ uint32_t ldsStack[QUERY_STACK_WORDS(CACHED) * RT_BLOCK];
    __shared__ float ldsKeys[RT64_RAY_LAYERS_MAX * RT_BLOCK];
    __shared__ uint8_t ldsSlots[RT64_RAY_LAYERS_MAX * RT_BLOCK];
    extern __shared__ u32x4_lds dynLds[];
    fill_cache<CACHED>(P, dynLds);
    TraceStack stk = lane_stack<CACHED>(P, ldsStack);
    if (CACHED) stk.use_cache(dynLds);
    // this lane's columns, stride RT_LANES, and its payload slots, stride RT_BLOCK (blockIdx.x < RT_GRID_BLOCKS: query_grid)
    const uint32_t column = (threadIdx.x >> 6) * RT64_RAY_LAYERS_MAX * RT_LANES + (threadIdx.x & 63u);
    const LdsF32Ptr keys = (LdsF32Ptr)(ldsKeys + column);
    const LdsU8Ptr slots = (LdsU8Ptr)(ldsSlots + column);
    const size_t firstSlot = (size_t)blockIdx.x * RT64_RAY_LAYERS_MAX * RT_BLOCK + threadIdx.x;
    const SlabU4Ptr slabA = (SlabU4Ptr)reinterpret_cast<uintptr_t>(slab) + firstSlot;
    const SlabU32Ptr slabB = (SlabU32Ptr)reinterpret_cast<uintptr_t>(slab + LAYER_SLAB_ENTRIES) + firstSlot;
    const uint64_t stride = query_stride();
    for (uint64_t i = query_first(); i < count; i += stride) {
        const QueryRay ray = load_ray(QUERY_IN(rays + i));
        const float lod = lods ? load_global(lods + i) : 0.0f;
        uint32_t nhits = 0;
        TraceCounts cnt; cnt.nodes = 0; cnt.tris = 0;
        const bool valid = query_ray_valid(ray.o, ray.d, ray.tmin, ray.tmax);
        if (valid)
            trace_ray<CACHED>(P, ray.o, ray.d, ray.tmin, ray.tmax, cullBackFaces != 0, stk,
                              [&](float t, float u, float v, uint32_t instance, uint32_t prim, float &tmax, uint32_t instFlags, float instDepthBias) -> bool {
                                  if (load_global(&P.instances[instance].cc.optTextureEdge)) {      // K2
                                      const float alpha = surface_alpha_at_lod(P, inst_view(P, instance), prim, u, v, lod);
                                      if (!(alpha > RT64_EDGE_ALPHA)) return false;          // H6: a cutout is neither stored nor shortens the ray
                                  }
                                  const float key = t - instDepthBias;                      // T2
                                  uint32_t hi = nhits < RT64_RAY_LAYERS_MAX ? nhits : RT64_RAY_LAYERS_MAX;
                                  uint32_t slot = nhits & (RT64_RAY_LAYERS_MAX - 1u);      // below 16 entries: the next unused payload slot
                                  while (hi > 0) {
                                      const float prev = keys[(hi - 1) * RT_LANES];
                                      if (!(key < prev)) break;
                                      const uint32_t prevSlot = slots[(hi - 1) * RT_LANES];
                                      if (hi < RT64_RAY_LAYERS_MAX) { keys[hi * RT_LANES] = prev; slots[hi * RT_LANES] = (uint8_t)prevSlot; }
                                      else slot = prevSlot & (RT64_RAY_LAYERS_MAX - 1u);  // the frame's scratch slot 16: the entry leaves the list and its payload slot is free
                                      hi--;
                                  }
                                  if (hi < RT64_RAY_LAYERS_MAX) {
                                      keys[hi * RT_LANES] = key;
                                      slots[hi * RT_LANES] = (uint8_t)(slot | ((instFlags & GPU_INST_OPAQUE) ? LAYER_OPAQUE_BIT : 0u));
                                      u32x4 a;
                                      a.x = __float_as_uint(t); a.y = __float_as_uint(u); a.z = __float_as_uint(v); a.w = instance;
                                      slabA[(size_t)slot * RT_BLOCK] = a;
                                      slabB[(size_t)slot * RT_BLOCK] = prim;
                                      ++nhits;
                                      if (hi == RT64_RAY_LAYERS_MAX - 1 && t < tmax) tmax = t;      // T4: the hit is committed
                                  }
                                  if (!(instFlags & GPU_INST_OPAQUE)) return false;
                                  const float lim = key + P.maxDepthBias;                   // T4
                                  if (lim < tmax) tmax = lim;
                                  return false;
                              }, cnt);
        keep_counts(P, cnt);
        // T3: the list ends with its first entry on an O1-opaque instance
        const uint32_t kept = nhits < RT64_RAY_LAYERS_MAX ? nhits : RT64_RAY_LAYERS_MAX;
        uint32_t length = 0; bool endsOpaque = false;
        while (length < kept && !endsOpaque) { endsOpaque = (slots[length * RT_LANES] & LAYER_OPAQUE_BIT) != 0u; length++; }
        const TraceCounts none = { 0u, 0u };
        for (uint32_t l = 0; l < maxLayers; l++) {          // T6: every record of the ray is written
            float t = INFINITY, u = 0.0f, v = 0.0f; uint32_t instance = 0xFFFFFFFFu, prim = 0xFFFFFFFFu;
            if (l < length) {
                const uint32_t slot = slots[l * RT_LANES] & (RT64_RAY_LAYERS_MAX - 1u);
                const u32x4 a = slabA[(size_t)slot * RT_BLOCK];
                t = __uint_as_float(a.x); u = __uint_as_float(a.y); v = __uint_as_float(a.z); instance = a.w;
                prim = slabB[(size_t)slot * RT_BLOCK];
            }
            STORE_QUERY_HIT(hits + ((uint64_t)l * count + i), t, u, v, instance, prim, none);
        }
        u32x4 r;
        r.x = length < maxLayers ? length : maxLayers;
        r.y = !valid ? 0u : (uint32_t)RT64_LAYERS_VALID | (endsOpaque ? (uint32_t)RT64_LAYERS_ENDS_OPAQUE : (length == RT64_RAY_LAYERS_MAX ? (uint32_t)RT64_LAYERS_FULL : 0u));
        r.z = cnt.nodes; r.w = cnt.tris;
        QUERY_OUT(layers + i)[0] = r;
    }
}

__global__ __launch_bounds__(RT_BLOCK) void layer_weight_kernel(FrameParams Pv, const RT64_RAY *rays, const RT64_RAY_HIT *hits, const float *lods, float *weights,
                                                                RT64_RAY_COVERAGE *coverage, uint64_t count, uint32_t maxLayers) {
    PRef P = *kernel_params(); (void)Pv;
    typedef float __attribute__((address_space(1))) *GFloatOut;
    const GFloatOut wout = (GFloatOut)reinterpret_cast<uintptr_t>(weights);
    const uint64_t stride = query_stride();
    for (uint64_t i = query_first(); i < count; i += stride) {
        const QueryRay ray = load_ray(QUERY_IN(rays + i));
        const float lod = lods ? load_global(lods + i) : 0.0f;
        const bool valid = query_ray_valid(ray.o, ray.d, ray.tmin, ray.tmax);
        float rem = 1.0f, refraction = 0.0f; uint32_t shaded = 0u, flags = valid ? (uint32_t)RT64_COVERAGE_VALID : 0u;
        bool open = valid;
        for (uint32_t l = 0; l < maxLayers; l++) {
            const uint64_t at = (uint64_t)l * count + i;
            float w = 0.0f;
            if (open) {
                const QueryHit h = load_hit(QUERY_IN(hits + at));
                if ((int32_t)h.instance < 0) open = false;                                             // the list's end
                else if (h.instance >= P.instanceCount || h.prim >= load_global(&P.instances[h.instance].triCount)) { flags |= RT64_COVERAGE_BAD_HIT; open = false; }
                else {
                    const InstView in = inst_view(P, h.instance);
                    float a = surface_alpha_at_lod(P, in, h.prim, h.u, h.v, lod);
                    if (in.cc.optTextureEdge && a > RT64_EDGE_ALPHA) a = 1.0f;                           // H6 (shade.h:481)
                    a = q_unorm8(a);                                                                   // shade.h:511
                    w = rem * a;                                                                       // passes.hip:123
                    if (w >= RT_EPSILON) {
                        rem *= (1.0f - a);                                                             // passes.hip:159
                        shaded++;
                        if (in.material.refractionFactor > RT_EPSILON) { refraction = rem; rem = 0.0f; flags |= RT64_COVERAGE_GLASS; }      // passes.hip:160
                    }
                    else w = 0.0f;                                                                     // the frame skips the layer
                    if (rem <= RT_EPSILON) { flags |= RT64_COVERAGE_COVERED; open = false; }           // passes.hip:172
                }
            }
            wout[at] = w;
        }
        u32x4 r;
        r.x = __float_as_uint(rem); r.y = __float_as_uint(refraction); r.z = shaded; r.w = flags;
        QUERY_OUT(coverage + i)[0] = r;
    }
}

}  // namespace

size_t ray_layer_slab_bytes() {
    return LAYER_SLAB_ENTRIES * (sizeof(u32x4) + sizeof(uint32_t));
}

hipError_t launch_layer_walk(const FrameParams &P, const void *rays, const void *lods, void *hits, void *layers, void *slab, uint64_t count, uint32_t maxLayers, uint32_t flags, hipStream_t s) {
    decltype(&layer_walk_kernel<false>) kernels[2] = { layer_walk_kernel<false>, layer_walk_kernel<true> };
    const uint32_t cull = (flags & RT64_RAY_FLAG_CULL_BACK_FACING) ? 1u : 0u;
    return launch_cached(kernels, P, count, 0, s, static_cast<const RT64_RAY *>(rays), static_cast<const float *>(lods), static_cast<RT64_RAY_HIT *>(hits),
                         static_cast<RT64_RAY_LAYERS *>(layers), static_cast<u32x4 *>(slab), count, maxLayers, cull);
}

hipError_t launch_layer_weight(const FrameParams &P, const void *rays, const void *hits, const void *lods, void *weights, void *coverage, uint64_t count, uint32_t maxLayers, hipStream_t s) {
    if (!count) return hipSuccess;
    hipLaunchKernelGGL(layer_weight_kernel, query_grid(count), dim3(RT_BLOCK), 0, s, P, static_cast<const RT64_RAY *>(rays), static_cast<const RT64_RAY_HIT *>(hits),
                       static_cast<const float *>(lods), static_cast<float *>(weights), static_cast<RT64_RAY_COVERAGE *>(coverage), count, maxLayers);
    return hipGetLastError();
}
