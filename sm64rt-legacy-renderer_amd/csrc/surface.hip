// surface.hip -- surface records for the hits of a ray query (RT64_ResolveViewRayHits, include/rt64_surface.h; rules A1-A9 in DESIGN.md 4).
//
// A resolve kernel of query_common.h: a streaming kernel beside the walk, not part of it.  Per record it reads 64 bytes (ray + hit, 16-byte loads), follows indices[3 prim + k] to three vertices, and writes 64 bytes
// (four 16-byte stores).  No LDS, no traversal stack, no spill slab.  The arithmetic is inst_view + get_vertex_data of shade.h -- the functions the frame's
// any-hit program (surface_anyhit_view) runs -- so position, normals and UV are the frame's own, before normal mapping and before quantisation; the loads of
// the InstView / VertexData fields a record does not use (material, previous transform, combiner inputs, texture slots) are dead code and not emitted.
//
// The instance differs per lane.  A wave whose hits all lie on one instance (coherent rays: most waves of a camera-like batch) reads that instance's two
// matrices, array pointers, vertex layout and triangle count into scalar registers; any other wave has every lane gather its own instance record (some 40
// dwords) with vector loads.  The any-hit's `waterfall` -- one scalar pass per distinct instance -- was measured as well: equal on coherent waves, 2.1 x
// slower on a shuffled batch over 66 instances.  hit_material_kernel repeats this block: behind a shared dispatcher (a function taking the
// per-hit code) both kernels compiled to other machine code, and this one ran 0.5 % slower on shuffled rays over 66 instances, so the block stays in the kernels.
#include "query_common.h"

namespace {

struct SurfaceRecord { f3 position, geometricNormal, shadingNormal; f2 uv; uint32_t flags; };

// A4-A8 for one real hit of instance `in`
DEV void surface_of_hit(const InstView &in, uint32_t prim, float u, float v, f3 rayDirW, SurfaceRecord &r) {
    const float b[3] = { 1.0f - u - v, u, v };
    VertexData vd;
    get_vertex_data(in, prim, b, false, vd);
    r.position = mul_point(in.objectToWorld.m, vd.vertexPosition);                              // curWorldPos of surface_anyhit_view
    r.geometricNormal = vd.triangleNormal;
    const bool back = dot3(vd.triangleNormal, rayDirW) > 0.0f;                                   // the frame's normalSign = -1
    const f3 n = normalize3(mul_vector(in.objectToWorldNormal.m, vd.vertexNormal));
    r.shadingNormal = back ? -n : n;
    r.flags = RT64_SURFACE_VALID | (back ? RT64_SURFACE_BACK_FACE : 0u);
    r.uv.x = 0.0f; r.uv.y = 0.0f;
    if (in.cc.vertexUV) { r.uv = vd.vertexUV; r.flags |= RT64_SURFACE_HAS_UV; }
}

__global__ __launch_bounds__(RT_BLOCK) void hit_surface_kernel(FrameParams Pv, const RT64_RAY *rays, const RT64_RAY_HIT *hits, RT64_RAY_SURFACE *surfaces, uint64_t count) {
    PRef P = *kernel_params(); (void)Pv;
    const uint64_t stride = query_stride();
    for (uint64_t i = query_first(); i < count; i += stride) {
        const QueryRay ray = load_ray(QUERY_IN(rays + i));          // (a record does not depend on the origin: that load is dead code)
        const QueryHit h = load_hit(QUERY_IN(hits + i));
        const f3 dir = mk3(ray.d[0], ray.d[1], ray.d[2]);
        const uint32_t instance = h.instance, prim = h.prim;
        const float u = h.u, v = h.v;
        // A2 / A3: the miss record; nothing below reads through an index that is out of range
        SurfaceRecord r;
        r.position = r.geometricNormal = r.shadingNormal = mk3s(0.0f); r.uv.x = r.uv.y = 0.0f;
        r.flags = (int32_t)instance < 0 ? 0u : (uint32_t)RT64_SURFACE_BAD_HIT;
        bool real = false;
        if (instance < P.instanceCount) {               // (unsigned: a negative instance is past the end)
            const uint32_t k0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)instance);
            if (__ballot(instance != k0) == 0ull) {     // the lanes in here agree: k0 is wave-uniform, inst_view's loads are scalar
                if (prim < load_const(&P.instances[k0].triCount)) { surface_of_hit(inst_view(P, k0), prim, u, v, dir, r); real = true; }
            }
            else if (prim < load_const(&P.instances[instance].triCount)) { surface_of_hit(inst_view(P, instance), prim, u, v, dir, r); real = true; }
        }
        u32x4 o0, o1, o2, o3;
        o0.x = __float_as_uint(r.position.x); o0.y = __float_as_uint(r.position.y); o0.z = __float_as_uint(r.position.z); o0.w = r.flags;
        o1.x = __float_as_uint(r.geometricNormal.x); o1.y = __float_as_uint(r.geometricNormal.y); o1.z = __float_as_uint(r.geometricNormal.z); o1.w = real ? instance : 0xFFFFFFFFu;
        o2.x = __float_as_uint(r.shadingNormal.x); o2.y = __float_as_uint(r.shadingNormal.y); o2.z = __float_as_uint(r.shadingNormal.z); o2.w = real ? prim : 0xFFFFFFFFu;
        o3.x = __float_as_uint(r.uv.x); o3.y = __float_as_uint(r.uv.y); o3.z = real ? __float_as_uint(h.t) : __float_as_uint(INFINITY); o3.w = 0u;
        GOut dst = QUERY_OUT(surfaces + i);
        dst[0] = o0; dst[1] = o1; dst[2] = o2; dst[3] = o3;
    }
}

}  // namespace

hipError_t launch_hit_surface(const FrameParams &P, const void *rays, const void *hits, void *surfaces, uint64_t count, hipStream_t s) {
    if (!count) return hipSuccess;
    hipLaunchKernelGGL(hit_surface_kernel, query_grid(count), dim3(RT_BLOCK), 0, s, P, static_cast<const RT64_RAY *>(rays), static_cast<const RT64_RAY_HIT *>(hits),
                       static_cast<RT64_RAY_SURFACE *>(surfaces), count);
    return hipGetLastError();
}
