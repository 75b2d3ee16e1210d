// alpha.h -- the alpha of one intersection, and nothing else of its material: what a walk that honours alpha (alpha_query.hip, rules K1-K10 in DESIGN.md 4)
// asks at every candidate.
//
// The two functions are the alpha halves of material_of_hit (material.hip) and of shadow_anyhit_alpha_view (shade.h): the same calls of get_vertex_data,
// tex_sample_level, color_formula and alpha_formula in the same order, so the values are those functions' values bit for bit (-ffp-contract=off: no
// operation is fused differently in one caller than in another).  What they leave out is everything a decision about alpha does not read: tangents, the
// colour lerps, the normal and specular samples, the object-to-world products, noise.  The compiler drops the unused outputs of get_vertex_data.
#pragma once
#include "shade.h"

#define RT64_EDGE_ALPHA 0.3f          // H6: a texture-edge shader cuts an intersection out iff !(alpha > RT64_EDGE_ALPHA)

// H3: the tail of tex_sample_grad behind its log2 -- clamp, then one level (POINT) or two blended (LINEAR).  `clamped` is the lod the sample was taken at.
DEV f4 tex_sample_lod(const TexView &t, float u, float v, float lod, uint32_t filter, uint32_t hAddr, uint32_t vAddr, float &clamped) {
    clamped = 0.0f;
    if (t.mips == 1) return tex_sample_level(t, u, v, 0, filter, hAddr, vAddr);
    const float maxLod = (float)(t.mips - 1);
    if (!(lod > 0.0f)) lod = 0.0f;                       // (NaN as well)
    if (lod > maxLod) lod = maxLod;
    clamped = lod;
    if (filter == 0) return tex_sample_level(t, u, v, (uint32_t)(int)(lod + 0.5f), filter, hAddr, vAddr);
    int l0 = (int)floorf(lod), l1 = l0 + 1 < (int)t.mips ? l0 + 1 : (int)t.mips - 1;
    float f = lod - (float)l0;
    f4 a = tex_sample_level(t, u, v, (uint32_t)l0, filter, hAddr, vAddr), b = tex_sample_level(t, u, v, (uint32_t)l1, filter, hAddr, vAddr);
    return mk4(a.x + f * (b.x - a.x), a.y + f * (b.y - a.y), a.z + f * (b.z - a.z), a.w + f * (b.w - a.w));
}

// The combiner's alpha for texel t0 (H5 / H10 before the multiplier)
DEV float combiner_alpha(const GpuCombiner &cc, const VertexData &vd, f4 t0) {
    const f4 t1 = mk4(1.0f, 0.0f, 1.0f, 1.0f);
    if (!cc.colorAlphaSame && cc.optAlpha) return alpha_formula(cc, vd, t0, t1);
    return color_formula(cc, cc.optAlpha, cc.optAlpha, vd, t0, t1).w;
}

// H5's alpha at H3's level, the value H6 holds against RT64_EDGE_ALPHA: RT64_ShadeViewRayHits flags the intersection RT64_MATERIAL_CUTOUT iff the shader has
// the texture-edge option and !(alpha > RT64_EDGE_ALPHA); the caller compares.
DEV float surface_alpha_at_lod(PRef P, const InstView &in, uint32_t prim, float u, float v, float lod) {
    const GpuCombiner &cc = in.cc;
    const float b[3] = { 1.0f - u - v, u, v };
    VertexData vd;
    get_vertex_data(in, prim, b, false, vd);
    f4 t0 = mk4(0, 0, 0, 0);
    if (cc.useTex0) {       // H4, mix included: the general colour formula scales by its third input's red, which can be the texel's
        const RT64_MATERIAL &mat = in.material;
        float unused;
        const f4 tex = tex_sample_lod(tex_view(P.textures + in.texDiffuse), vd.vertexUV.x, vd.vertexUV.y, lod, in.filter, in.hAddr, in.vAddr, unused);
        const float k = fmaxf(-mat.diffuseColorMix.w, 0.0f);
        t0 = mk4(lerpf(tex.x, mat.diffuseColorMix.x, k), lerpf(tex.y, mat.diffuseColorMix.y, k), lerpf(tex.z, mat.diffuseColorMix.z, k), tex.w);
    }
    return clampf(in.material.solidAlphaMultiplier * combiner_alpha(cc, vd, t0), 0.0f, 1.0f);
}

// H10: what a frame's shadow ray subtracts at this intersection before the noise factor (K7).  Negative = RT64_MATERIAL_SHADOW_CUTOUT, the intersection is ignored.
DEV float shadow_alpha_before_noise(PRef P, const InstView &in, uint32_t prim, float u, float v) {
    const GpuCombiner &cc = in.cc;
    const float b[3] = { 1.0f - u - v, u, v };
    VertexData vd;
    get_vertex_data(in, prim, b, false, vd);
    f4 t0 = mk4(0, 0, 0, 0);
    if (cc.useTex0) t0 = tex_sample_level(tex_view(P.textures + in.texDiffuse), vd.vertexUV.x, vd.vertexUV.y, 0, in.filter, in.hAddr, in.vAddr);
    float a = clampf(combiner_alpha(cc, vd, t0) * in.material.shadowAlphaMultiplier, 0.0f, 1.0f);
    if (cc.optTextureEdge) { if (a > RT64_EDGE_ALPHA) a = 1.0f; else return -1.0f; }
    return a;
}
