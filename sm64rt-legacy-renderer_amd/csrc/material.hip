// material.hip -- material records for the hits of a ray query (RT64_ShadeViewRayHits, include/rt64_material.h; rules H1-H12 in DESIGN.md 4).
//
// A resolve kernel of query_common.h beside hit_surface_kernel, not part of the walk.  Per record it reads 64 bytes (ray + hit, 16-byte loads) and one optional
// float (the lod), follows
// indices[3 prim + k] to three vertices, samples up to three textures and writes 64 bytes (four 16-byte stores).  No LDS, no traversal stack, no spill slab.
// The arithmetic is inst_view, get_vertex_data, color_formula, alpha_formula and tex_sample_level of shade.h -- the functions the frame's any-hit programs
// (surface_anyhit_view, shadow_anyhit_alpha_view) run, in their order -- so colour, normal, specular and shadow alpha are the frame's own before quantisation,
// with one difference by design: the mip level comes from the caller (H3), not from ray differentials a query does not have.
//
// The instance differs per lane and, unlike in surface.hip, steers control flow (combiner shape, filter, addressing, map flags).  A wave whose hits all lie on
// one instance reads that instance's record into scalar registers and branches uniformly; any other wave has every lane gather its own instance record with
// vector loads (the surface.hip scheme; DESIGN.md 4 has the figures against the any-hit's `waterfall`).
#include "query_common.h"
#include "alpha.h"

namespace {

struct MaterialRecord { f4 color; f3 shadingNormal, specular; float shadowAlpha, lod; uint32_t flags; };

// H2-H10 for one real hit of instance `in`: the body of surface_anyhit_view without pixel, frame number and quantisation, then shadow_anyhit_alpha_view's on the same vertex data
DEV void material_of_hit(PRef P, const InstView &in, uint32_t prim, float u, float v, f3 rayDirW, float lod, MaterialRecord &r) {
    const GpuCombiner &cc = in.cc;
    const RT64_MATERIAL &mat = in.material;
    const bool normalMap = (in.flags & GPU_INST_NORMAL_MAP) != 0, specularMap = (in.flags & GPU_INST_SPECULAR_MAP) != 0;
    const float b[3] = { 1.0f - u - v, u, v };
    const f4 mix = mk4(mat.diffuseColorMix.x, mat.diffuseColorMix.y, mat.diffuseColorMix.z, mat.diffuseColorMix.w);
    VertexData vd;
    get_vertex_data(in, prim, b, cc.vertexUV && normalMap, vd);
    r.flags = RT64_MATERIAL_VALID;
    r.lod = 0.0f;

    f4 t0 = mk4(0, 0, 0, 0), t0s = mk4(0, 0, 0, 0);
    const f4 t1 = mk4(1.0f, 0.0f, 1.0f, 1.0f);
    if (cc.useTex0) {                                                                       // H4, and H10's texel at level 0
        const TexView tv = tex_view(P.textures + in.texDiffuse);
        const f4 tex = tex_sample_lod(tv, vd.vertexUV.x, vd.vertexUV.y, lod, in.filter, in.hAddr, in.vAddr, r.lod);
        const float k = fmaxf(-mix.w, 0.0f);
        t0 = mk4(lerpf(tex.x, mix.x, k), lerpf(tex.y, mix.y, k), lerpf(tex.z, mix.z, k), tex.w);
        t0s = tex_sample_level(tv, vd.vertexUV.x, vd.vertexUV.y, 0, in.filter, in.hAddr, in.vAddr);
        r.flags |= RT64_MATERIAL_TEXTURED;
    }
    // H5, written out: result.w and sa are combiner_alpha(cc, vd, t0 / t0s) of alpha.h -- the same calls -- but taken from there the kernel compiles to other machine code
    f4 result; float sa;
    if (!cc.colorAlphaSame && cc.optAlpha) {
        result = color_formula(cc, false, true, vd, t0, t1);
        result.w = alpha_formula(cc, vd, t0, t1);
        sa = alpha_formula(cc, vd, t0s, t1);
    }
    else {
        result = color_formula(cc, cc.optAlpha, cc.optAlpha, vd, t0, t1);
        sa = color_formula(cc, cc.optAlpha, cc.optAlpha, vd, t0s, t1).w;
    }
    {
        const float k = fmaxf(mix.w, 0.0f);
        result.x = lerpf(result.x, mix.x, k); result.y = lerpf(result.y, mix.y, k); result.z = lerpf(result.z, mix.z, k);
    }
    result.w = clampf(mat.solidAlphaMultiplier * result.w, 0.0f, 1.0f);
    sa = clampf(sa * mat.shadowAlphaMultiplier, 0.0f, 1.0f);                                // H10
    if (cc.optTextureEdge) {                                                                // H6
        if (result.w > RT64_EDGE_ALPHA) result.w = 1.0f; else r.flags |= RT64_MATERIAL_CUTOUT;
        if (sa > RT64_EDGE_ALPHA) sa = 1.0f; else r.flags |= RT64_MATERIAL_SHADOW_CUTOUT;
    }
    if (cc.optNoise) r.flags |= RT64_MATERIAL_NOISE_ALPHA;                                  // H7
    r.color = result; r.shadowAlpha = sa;

    f3 vertexNormal = normalize3(mul_vector(in.objectToWorldNormal.m, vd.vertexNormal));    // H8
    const bool back = dot3(vd.triangleNormal, rayDirW) > 0.0f;
    const float normalSign = back ? -1.0f : 1.0f;
    if (back) r.flags |= RT64_MATERIAL_BACK_FACE;
    vertexNormal = vertexNormal * normalSign;
    float unused;
    if (cc.vertexUV && normalMap && in.texNormal >= 0) {
        const f3 tangent = normalize3(mul_vector(in.objectToWorldNormal.m, vd.vertexTangent)) * normalSign;
        const f3 binormal = normalize3(mul_vector(in.objectToWorldNormal.m, vd.vertexBinormal)) * normalSign;
        const float s = mat.uvDetailScale;
        const f4 tex = tex_sample_lod(tex_view(P.textures + in.texNormal), vd.vertexUV.x * s, vd.vertexUV.y * s, lod, in.filter, in.hAddr, in.vAddr, unused);
        const f3 nc = mk3(tex.x * 2.0f - 1.0f, tex.y * 2.0f - 1.0f, tex.z * 2.0f - 1.0f);
        vertexNormal = normalize3((vertexNormal * nc.z + tangent * nc.x) + binormal * nc.y);
        r.flags |= RT64_MATERIAL_NORMAL_MAPPED;
    }
    r.shadingNormal = vertexNormal;
    r.specular = mk3s(1.0f);                                                                // H9
    if (cc.vertexUV && specularMap && in.texSpecular >= 0) {
        const float s = mat.uvDetailScale;
        const f4 tex = tex_sample_lod(tex_view(P.textures + in.texSpecular), vd.vertexUV.x * s, vd.vertexUV.y * s, lod, in.filter, in.hAddr, in.vAddr, unused);
        r.specular = xyz(tex);
        r.flags |= RT64_MATERIAL_SPECULAR_MAPPED;
    }
}

__global__ __launch_bounds__(RT_BLOCK) void hit_material_kernel(FrameParams Pv, const RT64_RAY *rays, const RT64_RAY_HIT *hits, const float *lods, RT64_RAY_MATERIAL *materials, uint64_t count) {
    PRef P = *kernel_params(); (void)Pv;
    const uint64_t stride = query_stride();
    for (uint64_t i = query_first(); i < count; i += stride) {
        const GIn rsrc = QUERY_IN(rays + i), hsrc = QUERY_IN(hits + i);
        const QueryRay ray = load_ray(rsrc);          // (a record does not depend on the origin: that load is dead code)
        const QueryHit h = load_hit(hsrc);
        const float lod = lods ? lods[i] : 0.0f;
        const f3 dir = mk3(ray.d[0], ray.d[1], ray.d[2]);
        const uint32_t instance = h.instance, prim = h.prim;
        const float u = h.u, v = h.v;
        // H1: the miss record; nothing below reads through an index that is out of range
        MaterialRecord r;
        r.color = mk4(0, 0, 0, 0); r.shadingNormal = r.specular = mk3s(0.0f); r.shadowAlpha = r.lod = 0.0f;
        r.flags = (int32_t)instance < 0 ? 0u : (uint32_t)RT64_MATERIAL_BAD_HIT;
        bool real = false;
        if (instance < P.instanceCount) {               // (unsigned: a negative instance is past the end)
            const uint32_t k0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)instance);
            if (__ballot(instance != k0) == 0ull) {     // the lanes in here agree: k0 is wave-uniform, inst_view's loads are scalar and the combiner's branches uniform
                if (prim < load_const(&P.instances[k0].triCount)) { material_of_hit(P, inst_view(P, k0), prim, u, v, dir, lod, r); real = true; }
            }
            else if (prim < load_const(&P.instances[instance].triCount)) { material_of_hit(P, inst_view(P, instance), prim, u, v, dir, lod, r); real = true; }
        }
        u32x4 o0, o1, o2, o3;
        o0.x = __float_as_uint(r.color.x); o0.y = __float_as_uint(r.color.y); o0.z = __float_as_uint(r.color.z); o0.w = __float_as_uint(r.color.w);
        o1.x = __float_as_uint(r.shadingNormal.x); o1.y = __float_as_uint(r.shadingNormal.y); o1.z = __float_as_uint(r.shadingNormal.z); o1.w = r.flags;
        o2.x = __float_as_uint(r.specular.x); o2.y = __float_as_uint(r.specular.y); o2.z = __float_as_uint(r.specular.z); o2.w = __float_as_uint(r.shadowAlpha);
        o3.x = __float_as_uint(r.lod); o3.y = real ? instance : 0xFFFFFFFFu; o3.z = real ? prim : 0xFFFFFFFFu; o3.w = 0u;
        GOut dst = QUERY_OUT(materials + i);
        dst[0] = o0; dst[1] = o1; dst[2] = o2; dst[3] = o3;
    }
}

}  // namespace

hipError_t launch_hit_material(const FrameParams &P, const void *rays, const void *hits, const void *lods, void *materials, uint64_t count, hipStream_t s) {
    if (!count) return hipSuccess;
    hipLaunchKernelGGL(hit_material_kernel, query_grid(count), dim3(RT_BLOCK), 0, s, P, static_cast<const RT64_RAY *>(rays), static_cast<const RT64_RAY_HIT *>(hits),
                       static_cast<const float *>(lods), static_cast<RT64_RAY_MATERIAL *>(materials), count);
    return hipGetLastError();
}
