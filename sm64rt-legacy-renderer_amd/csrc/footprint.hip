// footprint.hip -- camera rays with their differentials and texture footprints for the hits of a ray query (RT64_GenerateViewCameraRays, RT64_FootprintViewRayHits,
// include/rt64_footprint.h; rules F1-F11 in DESIGN.md 4).
//
// camera_ray_kernel<DIFFS>: one pixel per lane on the grid-stride loop of query_common.h.  It reads 8 bytes (the pixel) or nothing (pixels = NULL: the index is the
// pixel), runs primary_ray + compute_ray_diffs of shade.h -- the functions the frame's ray generation runs -- and stores 32 bytes (the ray) and, with DIFFS, 64 more.
// It reads no scene memory beyond the frame parameters.
//
// hit_footprint_kernel<DIFFS>: a resolve kernel beside hit_surface_kernel.  Per record it reads 64 bytes (ray + hit) and, with DIFFS, the 64 of the differential,
// follows indices[3 prim + k] to three vertices, reads the table entries of up to three textures (size and mips: never a texel) and writes 64 bytes.  No LDS, no
// traversal stack, no spill slab.  inst_view and get_vertex_data are the frame's own.  The gradient block and the clamped-lod head are NOT functions in shade.h:
// they sit inline in surface_anyhit_view (shade.h, the lines under "propagateRayDiffs + computeBarycentricDifferentials + computeTextureDifferentials") and at
// the top of tex_sample_grad (from `float w0` to `if (lod > maxLod)`).  Factored into DEV functions that both sides call, they moved the machine code of 41 frame
// kernels (same instruction counts and registers, another schedule: profiles/footprint_kernel_identity.txt), so shade.h stays as it is and footprint_gradients and
// footprint_lod below restate those lines operation for operation; -ffp-contract=off makes the same operations give the same bits.
// tests/test_gpu_footprint_query.py holds the two together through the picture (F9).
//
// The choice between a wave-uniform and a per-lane instance read is written out as in hit_surface_kernel; surface.hip says why.
#include "query_common.h"

namespace {

template <bool DIFFS>
__global__ __launch_bounds__(RT_BLOCK) void camera_ray_kernel(FrameParams Pv, const uint2 *pixels, uint32_t firstPixel, RT64_RAY *rays, RT64_RAY_DIFFERENTIAL *diffs, uint64_t count) {
    PRef P = *kernel_params(); (void)Pv;
    const uint64_t stride = query_stride();
    const uint32_t width = (uint32_t)P.width;
    const bool listed = pixels != nullptr;          // (a kernel argument: uniform)
    for (uint64_t i = query_first(); i < count; i += stride) {
        uint32_t px, py;
        if (listed) { const uint2 p = pixels[i]; px = p.x; py = p.y; }
        else { const uint32_t n = firstPixel + (uint32_t)i; px = n % width; py = n / width; }          // F1 (the host refused more records than pixels: n fits 32 bits)
        f3 o, d; f2 ndc;
        primary_ray(P, px, py, o, d, ndc);                                        // F2
        u32x4 r0, r1;
        r0.x = __float_as_uint(o.x); r0.y = __float_as_uint(o.y); r0.z = __float_as_uint(o.z); r0.w = __float_as_uint(RT_RAY_MIN_DISTANCE);
        r1.x = __float_as_uint(d.x); r1.y = __float_as_uint(d.y); r1.z = __float_as_uint(d.z); r1.w = __float_as_uint(RT_RAY_MAX_DISTANCE);
        GOut rdst = QUERY_OUT(rays + i);
        rdst[0] = r0; rdst[1] = r1;
        if (DIFFS) {                                                              // F3: resolve_primary's call
            const f3 cU = mk3(P.cameraU[0], P.cameraU[1], P.cameraU[2]), cV = mk3(P.cameraV[0], P.cameraV[1], P.cameraV[2]), cW = mk3(P.cameraW[0], P.cameraW[1], P.cameraW[2]);
            const f3 nonNormRayDir = (cU * ndc.x + cV * ndc.y) + cW;
            f3 dDdx, dDdy;
            compute_ray_diffs(nonNormRayDir, cU, cV, P.resolution[2], P.resolution[3], dDdx, dDdy);
            u32x4 z, d2, d3;
            z.x = z.y = z.z = z.w = 0u;
            d2.x = __float_as_uint(dDdx.x); d2.y = __float_as_uint(dDdx.y); d2.z = __float_as_uint(dDdx.z); d2.w = 0u;
            d3.x = __float_as_uint(dDdy.x); d3.y = __float_as_uint(dDdy.y); d3.z = __float_as_uint(dDdy.z); d3.w = 0u;
            GOut ddst = QUERY_OUT(diffs + i);
            ddst[0] = z; ddst[1] = z; ddst[2] = d2; ddst[3] = d3;
        }
    }
}

struct FootprintRecord { f2 duvdx, duvdy; float lod, lodNormal, lodSpecular; uint32_t flags; f3 dPdx, dPdy; };

// surface_anyhit_view's gradient block, line for line (shade.h): propagate the differential to the hit (F5), then the barycentric differentials from the world-space
// corners times the UV edges (F6)
DEV void footprint_gradients(const VertexData &vd, bool hasUV, const RayDiff &payloadDiff, float t, f3 rayDirW, FootprintRecord &r) {
    f3 N = vd.triangleNormal;
    f3 dodx = payloadDiff.dOdx + payloadDiff.dDdx * t, dody = payloadDiff.dOdy + payloadDiff.dDdy * t;
    float rcpDN = s_rcp(dot3(rayDirW, N));
    float dtdx = -dot3(dodx, N) * rcpDN, dtdy = -dot3(dody, N) * rcpDN;
    dodx = dodx + rayDirW * dtdx; dody = dody + rayDirW * dtdy;
    r.dPdx = dodx; r.dPdy = dody;
    if (!hasUV) return;
    f3 e01 = vd.posW[1] - vd.posW[0], e02 = vd.posW[2] - vd.posW[0];
    f3 Nu = cross3(e02, N), Nv = cross3(e01, N);
    float du = dot3(Nu, e01), dv = dot3(Nv, e02);
    const float rdu = s_rcp(du), rdv = s_rcp(dv);
    f3 Lu = Nu * rdu, Lv = Nv * rdv;
    float dBdx_x = dot3(Lu, dodx), dBdx_y = dot3(Lv, dodx), dBdy_x = dot3(Lu, dody), dBdy_y = dot3(Lv, dody);
    float uv01x = vd.uv[1].x - vd.uv[0].x, uv01y = vd.uv[1].y - vd.uv[0].y, uv02x = vd.uv[2].x - vd.uv[0].x, uv02y = vd.uv[2].y - vd.uv[0].y;
    r.duvdx.x = dBdx_x * uv01x + dBdx_y * uv02x; r.duvdx.y = dBdx_x * uv01y + dBdx_y * uv02y;
    r.duvdy.x = dBdy_x * uv01x + dBdy_y * uv02x; r.duvdy.y = dBdy_x * uv01y + dBdy_y * uv02y;
}

// tex_sample_grad's head, line for line (shade.h): the clamped lod of one texture from its table entry (F7).  The comparisons are written so that a NaN or an
// infinite rho ends inside [0, mips - 1] (F8).
DEV float footprint_lod(const GpuTexture *entry, f2 ddx, f2 ddy) {
    const TexView t = tex_view(entry);
    if (t.mips == 1) return 0.0f;
    float w0 = (float)t.width, h0 = (float)t.height;
    float ax = ddx.x * w0, ay = ddx.y * h0, bx = ddy.x * w0, by = ddy.y * h0;
    float rho = fmaxf(s_sqrt(ax * ax + ay * ay), s_sqrt(bx * bx + by * by));
    float lod = rho > 0.0f ? log2f(rho) : 0.0f;
    float maxLod = (float)(t.mips - 1);
    if (!(lod > 0.0f)) lod = 0.0f;
    if (lod > maxLod) lod = maxLod;
    return lod;
}

// F5-F7 for one real hit of instance `in`
DEV void footprint_of_hit(PRef P, const InstView &in, uint32_t prim, float t, float u, float v, f3 rayDirW, const RayDiff &diff, FootprintRecord &r) {
    const GpuCombiner &cc = in.cc;
    const bool normalMap = (in.flags & GPU_INST_NORMAL_MAP) != 0, specularMap = (in.flags & GPU_INST_SPECULAR_MAP) != 0;
    const float b[3] = { 1.0f - u - v, u, v };
    VertexData vd;
    get_vertex_data(in, prim, b, false, vd);
    r.flags = RT64_FOOTPRINT_VALID;
    footprint_gradients(vd, cc.vertexUV != 0, diff, t, rayDirW, r);
    if (cc.vertexUV) r.flags |= RT64_FOOTPRINT_HAS_UV;
    // the frame leaves ddx / ddy at 0 unless the combiner reads texel 0, and hands THOSE to the normal and specular fetches: F7's quirk
    f2 ddx, ddy; ddx.x = ddx.y = ddy.x = ddy.y = 0.0f;
    // (the frame's block tests cc.useTex0 alone.  The other two conditions are defensive and cannot differ from it: the host derives vertexUV = useTex0 || useTex1
    // from the shader id and gives every instance a diffuse texture, so they only keep a table entry from being read through an index the host never writes.)
    if (cc.useTex0 && cc.vertexUV && in.texDiffuse >= 0) {
        ddx = r.duvdx; ddy = r.duvdy;
        r.lod = footprint_lod(P.textures + in.texDiffuse, ddx, ddy);
        r.flags |= RT64_FOOTPRINT_TEXTURED;
    }
    const float s = in.material.uvDetailScale;
    f2 gx, gy; gx.x = ddx.x * s; gx.y = ddx.y * s; gy.x = ddy.x * s; gy.y = ddy.y * s;
    if (cc.vertexUV && normalMap && in.texNormal >= 0) r.lodNormal = footprint_lod(P.textures + in.texNormal, gx, gy);
    if (cc.vertexUV && specularMap && in.texSpecular >= 0) r.lodSpecular = footprint_lod(P.textures + in.texSpecular, gx, gy);
}

template <bool DIFFS>
__global__ __launch_bounds__(RT_BLOCK) void hit_footprint_kernel(FrameParams Pv, const RT64_RAY *rays, const RT64_RAY_DIFFERENTIAL *diffs, const RT64_RAY_HIT *hits,
                                                                 RT64_RAY_FOOTPRINT *footprints, uint64_t count) {
    PRef P = *kernel_params(); (void)Pv;
    const uint64_t stride = query_stride();
    for (uint64_t i = query_first(); i < count; i += stride) {
        const QueryRay ray = load_ray(QUERY_IN(rays + i));          // (a record does not depend on the origin: that load is dead code)
        const QueryHit h = load_hit(QUERY_IN(hits + i));
        RayDiff diff;
        diff.dOdx = diff.dOdy = diff.dDdx = diff.dDdy = mk3s(0.0f);          // F4: diffs = NULL
        if (DIFFS) {
            const GIn dsrc = QUERY_IN(diffs + i);
            const u32x4 a = dsrc[0], b = dsrc[1], c = dsrc[2], d = dsrc[3];          // (the reserved words are not used)
            diff.dOdx = mk3(__uint_as_float(a.x), __uint_as_float(a.y), __uint_as_float(a.z)); diff.dOdy = mk3(__uint_as_float(b.x), __uint_as_float(b.y), __uint_as_float(b.z));
            diff.dDdx = mk3(__uint_as_float(c.x), __uint_as_float(c.y), __uint_as_float(c.z)); diff.dDdy = mk3(__uint_as_float(d.x), __uint_as_float(d.y), __uint_as_float(d.z));
        }
        const f3 dir = mk3(ray.d[0], ray.d[1], ray.d[2]);
        const uint32_t instance = h.instance, prim = h.prim;
        const float t = h.t, u = h.u, v = h.v;
        // F4: the miss record; nothing below reads through an index that is out of range
        FootprintRecord r;
        r.duvdx.x = r.duvdx.y = r.duvdy.x = r.duvdy.y = 0.0f; r.lod = r.lodNormal = r.lodSpecular = 0.0f; r.dPdx = r.dPdy = mk3s(0.0f);
        r.flags = (int32_t)instance < 0 ? 0u : (uint32_t)RT64_FOOTPRINT_BAD_HIT;
        bool real = false;
        if (instance < P.instanceCount) {               // (unsigned: a negative instance is past the end)
            const uint32_t k0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)instance);
            if (__ballot(instance != k0) == 0ull) {     // the lanes in here agree: k0 is wave-uniform, inst_view's loads are scalar and the branches on the shader uniform
                if (prim < load_const(&P.instances[k0].triCount)) { footprint_of_hit(P, inst_view(P, k0), prim, t, u, v, dir, diff, r); real = true; }
            }
            else if (prim < load_const(&P.instances[instance].triCount)) { footprint_of_hit(P, inst_view(P, instance), prim, t, u, v, dir, diff, r); real = true; }
        }
        u32x4 o0, o1, o2, o3;
        o0.x = __float_as_uint(r.duvdx.x); o0.y = __float_as_uint(r.duvdx.y); o0.z = __float_as_uint(r.duvdy.x); o0.w = __float_as_uint(r.duvdy.y);
        o1.x = __float_as_uint(r.lod); o1.y = __float_as_uint(r.lodNormal); o1.z = __float_as_uint(r.lodSpecular); o1.w = r.flags;
        o2.x = __float_as_uint(r.dPdx.x); o2.y = __float_as_uint(r.dPdx.y); o2.z = __float_as_uint(r.dPdx.z); o2.w = real ? instance : 0xFFFFFFFFu;
        o3.x = __float_as_uint(r.dPdy.x); o3.y = __float_as_uint(r.dPdy.y); o3.z = __float_as_uint(r.dPdy.z); o3.w = real ? prim : 0xFFFFFFFFu;
        GOut dst = QUERY_OUT(footprints + i);
        dst[0] = o0; dst[1] = o1; dst[2] = o2; dst[3] = o3;
    }
}

}  // namespace

hipError_t launch_camera_rays(const FrameParams &P, const void *pixels, uint64_t firstPixel, void *rays, void *diffs, uint64_t count, hipStream_t s) {
    if (!count) return hipSuccess;
    auto kernel = diffs ? camera_ray_kernel<true> : camera_ray_kernel<false>;
    hipLaunchKernelGGL(kernel, query_grid(count), dim3(RT_BLOCK), 0, s, P, static_cast<const uint2 *>(pixels), (uint32_t)firstPixel, static_cast<RT64_RAY *>(rays),
                       static_cast<RT64_RAY_DIFFERENTIAL *>(diffs), count);
    return hipGetLastError();
}

hipError_t launch_hit_footprint(const FrameParams &P, const void *rays, const void *diffs, const void *hits, void *footprints, uint64_t count, hipStream_t s) {
    if (!count) return hipSuccess;
    auto kernel = diffs ? hit_footprint_kernel<true> : hit_footprint_kernel<false>;
    hipLaunchKernelGGL(kernel, query_grid(count), dim3(RT_BLOCK), 0, s, P, static_cast<const RT64_RAY *>(rays), static_cast<const RT64_RAY_DIFFERENTIAL *>(diffs),
                       static_cast<const RT64_RAY_HIT *>(hits), static_cast<RT64_RAY_FOOTPRINT *>(footprints), count);
    return hipGetLastError();
}
