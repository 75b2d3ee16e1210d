// bounce.hip -- the frame's mirror and glass rays for the hits of a ray query, and mirror chains in one walk (RT64_BounceViewRayHits, RT64_TraceViewRayMirrorChains,
// include/rt64_bounce.h; rules R1-R12 in DESIGN.md 4).
//
// Two kernels of query_common.h:
//   hit_bounce_kernel    a resolve kernel: per record 64 bytes in (ray + hit, 16-byte loads) and one optional float (the lod); it rebuilds the shading normal as
//                        hit_material_kernel does (R3), takes the point on the ray (R2), and writes up to 96 bytes -- the record, the reflected ray (R4), the refracted ray
//                        (R5) -- with 16-byte stores.  A NULL output array skips its stores (the pointers are kernel arguments: the branch is wave-uniform).  No LDS, no
//                        stack.  The hit's own instance is read by material.hip's scheme: scalar loads for a wave whose hits agree on it, per-lane inst_view otherwise.
//   mirror_chain_kernel  a walk kernel: per ray up to `depth` segments.  Segment 0 is alpha_query_kernel<false, *>'s walk of the ray at its lod, every later one that walk
//                        of the previous segment's reflected ray at lod 0 while the hit is a mirror (R7).  fill_cache / lane_stack / use_cache are alpha_query_kernel's;
//                        the K2 handler is its own, statement for statement, with the per-lane gather (alpha_query.hip's head comment has the open defect of `waterfall`).
//                        A lane whose chain has ended idles until the wave's longest chain ends and stores the miss records of its unreached segments itself.
// Both build a record with the one function bounce_of_hit, which calls get_vertex_data, tex_sample_lod, reflect3 and fresnel_reflect_amount of shade.h / alpha.h /
// device_math.h in the order of material_of_hit and reflection_kernel; with -ffp-contract=off a chain's segment is therefore byte for byte what the one-step calls give.
// hlsl_refract restates passes.hip:1083-1088 (a .hip file's function is not reachable from here, and passes.hip stays untouched).
#include "query_common.h"
#include "alpha.h"

namespace {

DEV f3 hlsl_refract(f3 i, f3 n, float eta, bool &total) {          // passes.hip:1083-1088; total: the k < 0 branch was taken (RT64_BOUNCE_TOTAL_INTERNAL)
    float cosi = dot3(n, i);
    float k = 1.0f - eta * eta * (1.0f - cosi * cosi);
    total = k < 0.0f;
    if (total) return mk3s(0.0f);
    return i * eta - n * (eta * cosi + sqrtf(k));
}

struct BounceRecord { f3 position, reflected, refracted; float fresnel, reflectionFactor, refractionFactor; uint32_t flags; };

DEV void bounce_miss(BounceRecord &r, uint32_t flags) {          // R1
    r.position = r.reflected = r.refracted = mk3s(0.0f); r.fresnel = r.reflectionFactor = r.refractionFactor = 0.0f; r.flags = flags;
}

// R2-R6 for one real hit of instance `in`: material_of_hit's normal chain (H8), then the frame's point and its two secondary directions
DEV void bounce_of_hit(PRef P, const InstView &in, uint32_t prim, float t, float u, float v, f3 rayOrigin, f3 rayDirection, float lod, BounceRecord &r) {
    const GpuCombiner &cc = in.cc;
    const RT64_MATERIAL &mat = in.material;
    const bool normalMap = (in.flags & GPU_INST_NORMAL_MAP) != 0;
    const float b[3] = { 1.0f - u - v, u, v };
    VertexData vd;
    get_vertex_data(in, prim, b, cc.vertexUV && normalMap, vd);
    r.flags = RT64_BOUNCE_VALID;
    f3 vertexNormal = normalize3(mul_vector(in.objectToWorldNormal.m, vd.vertexNormal));    // H8
    const bool back = dot3(vd.triangleNormal, rayDirection) > 0.0f;
    const float normalSign = back ? -1.0f : 1.0f;
    if (back) r.flags |= RT64_BOUNCE_BACK_FACE;
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
    const float dist = t - mat.depthBias;                                                    // the hit record's sort key (shade.h:509) ...
    r.position = rayOrigin + rayDirection * (dist + mat.depthBias);                          // R2: ... and passes.hip:129 on it, rounding for rounding
    r.reflected = reflect3(rayDirection, vertexNormal);                                      // R4: passes.hip:1200
    bool total;
    r.refracted = hlsl_refract(rayDirection, vertexNormal, mat.refractionFactor, total);     // R5: passes.hip:1112
    if (total) r.flags |= RT64_BOUNCE_TOTAL_INTERNAL;
    r.reflectionFactor = mat.reflectionFactor; r.refractionFactor = mat.refractionFactor;
    r.fresnel = 0.0f;
    if (mat.reflectionFactor > RT_EPSILON) {                                                 // R6: passes.hip:138-139
        r.flags |= RT64_BOUNCE_MIRROR;
        r.fresnel = fresnel_reflect_amount(vertexNormal, rayDirection, mat.reflectionFactor, mat.reflectionFresnelFactor);
    }
    if (mat.refractionFactor > RT_EPSILON) r.flags |= RT64_BOUNCE_GLASS;
}

// the three stores of a record; `real`: the hit was resolved (else the rays are 32 zero bytes and the indices -1).  A macro for the reason STORE_QUERY_HIT is one.
#define STORE_BOUNCE(outB, outR, outT, at, r, real, instance, prim, nodes, tris) do { \
        if (outB) { \
            u32x4 b0_, b1_; \
            b0_.x = __float_as_uint((r).fresnel); b0_.y = __float_as_uint((r).reflectionFactor); b0_.z = __float_as_uint((r).refractionFactor); b0_.w = (r).flags; \
            b1_.x = (real) ? (instance) : 0xFFFFFFFFu; b1_.y = (real) ? (prim) : 0xFFFFFFFFu; b1_.z = (nodes); b1_.w = (tris); \
            GOut dst_ = QUERY_OUT((outB) + (at)); dst_[0] = b0_; dst_[1] = b1_; \
        } \
        const uint32_t tmin_ = (real) ? __float_as_uint(RT_RAY_MIN_DISTANCE) : 0u, tmax_ = (real) ? __float_as_uint(RT_RAY_MAX_DISTANCE) : 0u; \
        if (outR) { \
            u32x4 r0_, r1_; \
            r0_.x = __float_as_uint((r).position.x); r0_.y = __float_as_uint((r).position.y); r0_.z = __float_as_uint((r).position.z); r0_.w = tmin_; \
            r1_.x = __float_as_uint((r).reflected.x); r1_.y = __float_as_uint((r).reflected.y); r1_.z = __float_as_uint((r).reflected.z); r1_.w = tmax_; \
            GOut dst_ = QUERY_OUT((outR) + (at)); dst_[0] = r0_; dst_[1] = r1_; \
        } \
        if (outT) { \
            u32x4 r0_, r1_; \
            r0_.x = __float_as_uint((r).position.x); r0_.y = __float_as_uint((r).position.y); r0_.z = __float_as_uint((r).position.z); r0_.w = tmin_; \
            r1_.x = __float_as_uint((r).refracted.x); r1_.y = __float_as_uint((r).refracted.y); r1_.z = __float_as_uint((r).refracted.z); r1_.w = tmax_; \
            GOut dst_ = QUERY_OUT((outT) + (at)); dst_[0] = r0_; dst_[1] = r1_; \
        } \
    } while (0)

// carryCounters: the hits come from the walk of the same call (RT64_TraceViewRayBounces) and the record takes their counters (R8); otherwise they are 0
__global__ __launch_bounds__(RT_BLOCK) void hit_bounce_kernel(FrameParams Pv, const RT64_RAY *rays, const RT64_RAY_HIT *hits, const float *lods, RT64_RAY_BOUNCE *bounces,
                                                              RT64_RAY *reflected, RT64_RAY *refracted, uint64_t count, uint32_t carryCounters) {
    PRef P = *kernel_params(); (void)Pv;
    const uint64_t stride = query_stride();
    for (uint64_t i = query_first(); i < count; i += stride) {
        const GIn rsrc = QUERY_IN(rays + i), hsrc = QUERY_IN(hits + i);
        const QueryRay ray = load_ray(rsrc);
        const u32x4 h0 = hsrc[0], h1 = hsrc[1];
        const float lod = lods ? load_global(lods + i) : 0.0f;
        const f3 origin = mk3(ray.o[0], ray.o[1], ray.o[2]), dir = mk3(ray.d[0], ray.d[1], ray.d[2]);
        const uint32_t instance = h0.w, prim = h1.x;
        const float t = __uint_as_float(h0.x), u = __uint_as_float(h0.y), v = __uint_as_float(h0.z);
        // R1: the miss record; nothing below reads through an index that is out of range
        BounceRecord r;
        bounce_miss(r, (int32_t)instance < 0 ? 0u : (uint32_t)RT64_BOUNCE_BAD_HIT);
        bool real = false;
        if (instance < P.instanceCount) {               // (unsigned: a negative instance is past the end)
            const uint32_t k0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)instance);
            if (__ballot(instance != k0) == 0ull) {     // the lanes in here agree: k0 is wave-uniform, inst_view's loads are scalar and the map branch uniform
                if (prim < load_const(&P.instances[k0].triCount)) { bounce_of_hit(P, inst_view(P, k0), prim, t, u, v, origin, dir, lod, r); real = true; }
            }
            else if (prim < load_const(&P.instances[instance].triCount)) { bounce_of_hit(P, inst_view(P, instance), prim, t, u, v, origin, dir, lod, r); real = true; }
        }
        const uint32_t nodes = carryCounters ? h1.y : 0u, tris = carryCounters ? h1.z : 0u;
        STORE_BOUNCE(bounces, reflected, refracted, i, r, real, instance, prim, nodes, tris);
    }
}

template <bool CACHED>
__global__ __launch_bounds__(RT_BLOCK) void mirror_chain_kernel(FrameParams Pv, const RT64_RAY *rays, const float *lods, RT64_RAY_HIT *hits, RT64_RAY_BOUNCE *bounces,
                                                                uint64_t count, uint32_t depth, uint32_t cullBackFaces) {
    PRef P = *kernel_params(); (void)Pv;
    __shared__ uint32_t ldsStack[QUERY_STACK_WORDS(CACHED) * RT_BLOCK];
    extern __shared__ u32x4_lds dynLds[];
    fill_cache<CACHED>(P, dynLds);
    TraceStack stk = lane_stack<CACHED>(P, ldsStack);
    if (CACHED) stk.use_cache(dynLds);
    const uint64_t stride = query_stride();
    RT64_RAY *const noRays = nullptr;
    for (uint64_t i = query_first(); i < count; i += stride) {
        QueryRay ray = load_ray(QUERY_IN(rays + i));
        float lod = lods ? load_global(lods + i) : 0.0f;
        bool alive = true;
        for (uint32_t s = 0; s < depth; s++) {
            float ht = INFINITY, hu = 0.0f, hv = 0.0f; uint32_t hInstance = 0xFFFFFFFFu, hPrim = 0xFFFFFFFFu;
            TraceCounts cnt; cnt.nodes = 0; cnt.tris = 0;
            BounceRecord r;
            bounce_miss(r, 0u);
            bool real = false;
            if (alive) {
                if (query_ray_valid(ray.o, ray.d, ray.tmin, ray.tmax))
                    trace_ray<CACHED>(P, ray.o, ray.d, ray.tmin, ray.tmax, cullBackFaces != 0, stk,
                                      [&](float t, float u, float v, uint32_t instance, uint32_t prim, float &tm, uint32_t, float) -> bool {
                                          if (load_global(&P.instances[instance].cc.optTextureEdge)) {      // K2: every other instance commits as in Q2
                                              const float alpha = surface_alpha_at_lod(P, inst_view(P, instance), prim, u, v, lod);
                                              if (!(alpha > RT64_EDGE_ALPHA)) return false;          // H6: a cutout neither commits nor shortens the ray
                                          }
                                          ht = t; hu = u; hv = v; hInstance = instance; hPrim = prim;
                                          tm = t;
                                          return false;
                                      }, cnt);
                keep_counts(P, cnt);
                // the walk's own hit: its instance and primitive are in range
                if (hInstance < P.instanceCount && hPrim < load_global(&P.instances[hInstance].triCount)) {
                    bounce_of_hit(P, inst_view(P, hInstance), hPrim, ht, hu, hv, mk3(ray.o[0], ray.o[1], ray.o[2]), mk3(ray.d[0], ray.d[1], ray.d[2]), lod, r);
                    real = true;
                }
            }
            const bool next = real && (r.flags & RT64_BOUNCE_MIRROR) != 0u && s + 1u < depth;      // R7
            if (next) r.flags |= RT64_BOUNCE_CONTINUED;
            const uint64_t at = (uint64_t)s * count + i;
            STORE_QUERY_HIT(hits + at, ht, hu, hv, hInstance, hPrim, cnt);
            STORE_BOUNCE(bounces, noRays, noRays, at, r, real, hInstance, hPrim, cnt.nodes, cnt.tris);
            alive = next;
            // the next segment's ray: R4's, at lod 0 (a frame's secondary rays carry no differentials)
            ray.o[0] = r.position.x; ray.o[1] = r.position.y; ray.o[2] = r.position.z; ray.d[0] = r.reflected.x; ray.d[1] = r.reflected.y; ray.d[2] = r.reflected.z;
            ray.tmin = RT_RAY_MIN_DISTANCE; ray.tmax = RT_RAY_MAX_DISTANCE;
            lod = 0.0f;
        }
    }
}

}  // namespace

hipError_t launch_hit_bounce(const FrameParams &P, const void *rays, const void *hits, const void *lods, void *bounces, void *reflected, void *refracted, uint64_t count, bool carryCounters, hipStream_t s) {
    if (!count) return hipSuccess;
    hipLaunchKernelGGL(hit_bounce_kernel, query_grid(count), dim3(RT_BLOCK), 0, s, P, static_cast<const RT64_RAY *>(rays), static_cast<const RT64_RAY_HIT *>(hits),
                       static_cast<const float *>(lods), static_cast<RT64_RAY_BOUNCE *>(bounces), static_cast<RT64_RAY *>(reflected), static_cast<RT64_RAY *>(refracted), count,
                       carryCounters ? 1u : 0u);
    return hipGetLastError();
}

hipError_t launch_mirror_chain(const FrameParams &P, const void *rays, const void *lods, void *hits, void *bounces, uint64_t count, uint32_t depth, uint32_t flags, hipStream_t s) {
    decltype(&mirror_chain_kernel<false>) kernels[2] = { mirror_chain_kernel<false>, mirror_chain_kernel<true> };
    const uint32_t cull = (flags & RT64_RAY_FLAG_CULL_BACK_FACING) ? 1u : 0u;
    return launch_cached(kernels, P, count, 0, s, static_cast<const RT64_RAY *>(rays), static_cast<const float *>(lods), static_cast<RT64_RAY_HIT *>(hits),
                         static_cast<RT64_RAY_BOUNCE *>(bounces), count, depth, cull);
}
