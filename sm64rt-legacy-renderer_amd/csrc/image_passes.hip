// image_passes.hip -- the kernels of the frame's passes that are compiled ONCE (passes.hip holds the ray kernels that exist twice):
//   scene_cache_image      the LDS scene cache's contents, assembled in HBM once per table change
//   primary_trace          <- PrimaryRayGen (shaders/PrimaryRayGen.hlsl:31-198), visibility only: it runs no shading code, so it has no "simple" twin
//   gaussian               <- GaussianFilterRGB3x3CS.hlsl:21-82
//   compose_post           <- ComposePS.hlsl:18-37 + PostProcessPS.hlsl:13-36 (fused: one read of the G-buffer)
//   post_process, debug_view, indirect_constant, spp_accumulate, tile_order, apply_reflection_state, clear_final, stack_slab_init
// and the host's counts of tiles and spill slabs.  Image-space kernels: workgroups of 256 threads over 32 x 8 pixels (image_grid).
#include "pass_common.h"

namespace {

DEV uint32_t cache_child_ref(uint32_t c) { return (c & RT64_LEAF_BIT) ? (c == RT64_NO_CHILD ? c : (0xFFFF8000u | (c & RT_CACHE_INDEX_MASK))) : c; }
DEV void copy_cache_nodes(const GpuNode *nodes, uint32_t count, u32x4 *dst) {      // word 3 of a node = (left, right, parent, pad): the child references become 16-bit
    typedef const u32x4 __attribute__((address_space(1))) *G4;
    G4 src = reinterpret_cast<G4>(reinterpret_cast<uintptr_t>(nodes));
    for (uint32_t t = threadIdx.x; t < 4u * count; t += blockDim.x) {
        u32x4 w = src[t];
        if ((t & 3u) == 3u) { w.x = cache_child_ref(w.x); w.y = cache_child_ref(w.y); }
        dst[t] = w;
    }
}
// blasOnly: the head (instance records + TLAS nodes) arrived with the table upload, written by the host (View::update: hostCache); only the BLAS node arrays are copied
__global__ __launch_bounds__(RT_BLOCK) void scene_cache_image_kernel(const GpuInstance *instances, const uint32_t *tlasIndex, const GpuNode *tlasNodes, uint32_t m, u32x4 *cache, int blasOnly) {
    typedef u32x4 W4;
    const uint32_t T = blockDim.x, tid = threadIdx.x;

    for (uint32_t k = tid; k < m && !blasOnly; k += T) {
        const uint32_t inst = tlasIndex[k];
        const GpuInstance &in = instances[inst];
        const float *M = in.worldToObject;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            W4 w; w.x = __float_as_uint(M[c]); w.y = __float_as_uint(M[4 + c]); w.z = __float_as_uint(M[8 + c]); w.w = __float_as_uint(M[12 + c]);
            cache[4 * k + c] = w;
        }
        const uint64_t tp = reinterpret_cast<uint64_t>(in.tris);
        W4 info; info.x = inst | ((in.flags & 0xFFu) << 8) | (in.cacheNodeOffset << 16); info.y = __float_as_uint(in.material.depthBias); info.z = (uint32_t)tp; info.w = (uint32_t)(tp >> 32);
        cache[4 * k + 3] = info;
    }
    if (!blasOnly) copy_cache_nodes(tlasNodes, m > 1 ? m - 1 : 1u, cache + 4 * m);
    for (uint32_t k = 0; k < m; k++) {                       // uniform: every thread walks the same instance list
        const GpuInstance &in = instances[tlasIndex[k]];
        copy_cache_nodes(in.nodes, in.triCount > 1 ? in.triCount - 1 : 1u, cache + in.cacheNodeOffset);
    }
}

// ---- primary visibility --------------------------------------------------------------------------------------------------

template <bool KLIST, bool CACHED = false>
__global__ __launch_bounds__(RT_BLOCK, KLIST ? 2 : TRACE_WAVES) void primary_trace_kernel(FrameParams Pv, ViewImages Iv, int32_t *hitInstance) {
    PRef P = *kernel_params(); IRef I = *kernel_images(); (void)Pv; (void)Iv; (void)I;
    __shared__ uint32_t ldsStack[stack_words(CACHED) * RT_BLOCK];
    extern __shared__ u32x4_lds dynLds[];
    if (CACHED) fill_scene_cache(P, dynLds);
    ShadeEnv env; traversal_env<CACHED>(P, env, ldsStack, dynLds);
    uint32_t rays = 0;
    const uint32_t tiles = tile_count(P);
    for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        PRef P = *kernel_params_here(); IRef I = *kernel_images_here();      // this trip's view of the frame constants and the image table (read where used, never carried across trips)
        Pixel p = tile_pixel(P, tile);
        if (!p.valid) continue;
        f3 o, d; f2 ndc;
        primary_ray(P, p.x, p.y, o, d, ndc);
        const size_t i = (size_t)p.y * (size_t)P.width + p.x;
        RayDiff rayDiff;
        if (KLIST) {    // the texture-edge any-hit samples with the primary ray differentials (PrimaryRayGen.hlsl:55-59)
            f3 cU = mk3(P.cameraU[0], P.cameraU[1], P.cameraU[2]), cV = mk3(P.cameraV[0], P.cameraV[1], P.cameraV[2]), cW = mk3(P.cameraW[0], P.cameraW[1], P.cameraW[2]);
            rayDiff.dOdx = mk3s(0.0f); rayDiff.dOdy = mk3s(0.0f);
            compute_ray_diffs((cU * ndc.x + cV * ndc.y) + cW, cU, cV, P.resolution[2], P.resolution[3], rayDiff.dDdx, rayDiff.dDdy);
        }
        SurfaceHit h;
        const uint32_t nhits = trace_surface<KLIST, CACHED>(P, env, I, i, o, d, rayDiff, p.x, p.y, h);
        rays++;
        uint4 rec;
        if (KLIST) {
            I.klistCount[i] = nhits;
            if (nhits) {
                const uint4 a = I.klistA[i]; const uint2 b = I.klistB[i];
                rec = make_uint4(b.x, a.y, a.z, a.w); hitInstance[i] = (int32_t)b.y;
            }
            else { rec.x = rec.y = rec.z = rec.w = 0xFFFFFFFFu; hitInstance[i] = -1; }
        }
        else if (h.hit) { rec.x = __float_as_uint(h.t); rec.y = __float_as_uint(h.u); rec.z = __float_as_uint(h.v); rec.w = h.prim; hitInstance[i] = (int32_t)h.instance; }
        else { rec.x = rec.y = rec.z = rec.w = 0xFFFFFFFFu; hitInstance[i] = -1; }
        reinterpret_cast<uint4 *>(I.primaryHit)[i] = rec;
    }
    flush_env(P, env, PASS_PRIMARY_TRACE, CTR_PRIMARY, rays);
}

// ---- GaussianFilterRGB3x3CS ------------------------------------------------------------------------------------------------

DEV f3 bilinear_clamp_rgb(const uint16_t *img, int w, int h, float u, float v) {   // LINEAR + CLAMP static sampler, rt64_device.cpp:737-742
    float x = u * (float)w - 0.5f, y = v * (float)h - 0.5f;
    float x0f = floorf(x), y0f = floorf(y), fx = x - x0f, fy = y - y0f;
    int x0 = (int)x0f, y0 = (int)y0f, x1 = x0 + 1, y1 = y0 + 1;
    x0 = x0 < 0 ? 0 : (x0 >= w ? w - 1 : x0); x1 = x1 < 0 ? 0 : (x1 >= w ? w - 1 : x1);
    y0 = y0 < 0 ? 0 : (y0 >= h ? h - 1 : y0); y1 = y1 < 0 ? 0 : (y1 >= h ? h - 1 : y1);
    f3 c00 = xyz(load_rgba16f(img, (size_t)y0 * w + x0)), c10 = xyz(load_rgba16f(img, (size_t)y0 * w + x1));
    f3 c01 = xyz(load_rgba16f(img, (size_t)y1 * w + x0)), c11 = xyz(load_rgba16f(img, (size_t)y1 * w + x1));
    f3 top = lerp3(c00, c10, fx), bot = lerp3(c01, c11, fx);
    return lerp3(top, bot, fy);
}

__global__ __launch_bounds__(256) void gaussian_kernel(const uint16_t *in, uint16_t *out, int w, int h, int y0, int y1) {
    const int x = blockIdx.x * 32 + (threadIdx.x & 31), y = y0 + blockIdx.y * 8 + (threadIdx.x >> 5);
    if (x >= w || y >= y1) return;
    const float texelX = 1.0f / (float)w, texelY = 1.0f / (float)h;
    const float k00 = 0.077847f, k01 = 0.123317f, k11 = 0.195346f;
    float wt[4];
    const bool xl = x == 0, xr = x == w - 1, yt = y == 0, yb = y == h - 1;
    if (x > 0 && y > 0 && x < w - 1 && y < h - 1) { wt[0] = k00 + k01 + k01 + k11; wt[1] = k00 + k01; wt[2] = k00 + k01; wt[3] = k00; }
    else if (xl && yt) { wt[0] = k11 / 0.519827f; wt[1] = k01 / 0.519827f; wt[2] = k01 / 0.519827f; wt[3] = k00 / 0.519827f; }
    else if (xr && yt) { wt[0] = (k01 + k11) / 0.519827f; wt[1] = 0.0f; wt[2] = 0.201164f / 0.519827f; wt[3] = 0.0f; }
    else if (xl && yb) { wt[0] = (k01 + k11) / 0.519827f; wt[1] = (k00 + k01) / 0.519827f; wt[2] = 0.0f; wt[3] = 0.0f; }
    else if (xr && yb) { wt[0] = (k00 + k01 + k01 + k11) / 0.519827f; wt[1] = wt[2] = wt[3] = 0.0f; }
    else if (xl) { wt[0] = (k01 + k11) / 0.720991f; wt[1] = (k00 + k01) / 0.720991f; wt[2] = k01 / 0.720991f; wt[3] = k00 / 0.720991f; }
    else if (xr) { wt[0] = (k00 + k01 + k01 + k11) / 0.720991f; wt[1] = 0.0f; wt[2] = (k00 + k01) / 0.720991f; wt[3] = 0.0f; }
    else if (yt) { wt[0] = (k01 + k11) / 0.720991f; wt[1] = k01 / 0.720991f; wt[2] = (k00 + k01) / 0.720991f; wt[3] = k00 / 0.720991f; }
    else { wt[0] = (k00 + k01 + k01 + k11) / 0.720991f; wt[1] = (k00 + k01) / 0.720991f; wt[2] = 0.0f; wt[3] = 0.0f; }
    const float off[3][2] = { { 0.5f + -k01 / (k01 + k11), 0.5f + -k01 / (k01 + k11) }, { 0.5f + 1.0f, 0.5f + -k00 / (k00 + k01) }, { 0.5f + -k00 / (k00 + k01), 0.5f + 1.0f } };
    f3 smp[4];
#pragma unroll
    for (int k = 0; k < 3; k++) smp[k] = bilinear_clamp_rgb(in, w, h, ((float)x + off[k][0]) * texelX, ((float)y + off[k][1]) * texelY);
    smp[3] = (x + 1 < w && y + 1 < h) ? xyz(load_rgba16f(in, (size_t)(y + 1) * w + (x + 1))) : mk3s(0.0f);
    const size_t i = (size_t)y * w + x;
    f4 old = load_rgba16f(out, i);
    store_rgba16f(out, i, smp[0].x * wt[0] + smp[1].x * wt[1] + smp[2].x * wt[2] + smp[3].x * wt[3],
                  smp[0].y * wt[0] + smp[1].y * wt[1] + smp[2].y * wt[2] + smp[3].y * wt[3],
                  smp[0].z * wt[0] + smp[1].z * wt[1] + smp[2].z * wt[2] + smp[3].z * wt[3], old.w);
}

// ---- ComposePS + PostProcessPS (fused) -------------------------------------------------------------------------------------

// LEAN: direct light straight from the raw accumulation, constant ambient for the indirect term (giSamples == 0), and no
// reflection / refraction / transparent reads -- all of them are exact zeros on a lean frame.
template <bool LEAN>
__global__ __launch_bounds__(256) void compose_post_kernel(FrameParams Pv, ViewImages Iv, int cur, int writeFinal) {
    PRef P = *kernel_params(); IRef I = *kernel_images(); (void)Pv; (void)Iv; (void)I;
    const int x = blockIdx.x * 32 + (threadIdx.x & 31), y = P.tileY0 + blockIdx.y * 8 + (threadIdx.x >> 5);
    if (x >= P.width || y >= P.tileY1 || !row_owned(P, y)) return;
    const size_t i = (size_t)y * (size_t)P.width + x;
    f4 d = load_rgba8(I.diffuse, i);
    f3 result;
    if (d.w > RT_EPSILON) {
        f3 diffuse = xyz(d);
        f3 direct, indirect;
        if (LEAN) {
            direct = xyz(load_rgba16f(I.directLight[cur], i));
            indirect = mk3(q_f16(P.ambientBaseColor[0] + P.ambientNoGIColor[0]), q_f16(P.ambientBaseColor[1] + P.ambientNoGIColor[1]), q_f16(P.ambientBaseColor[2] + P.ambientNoGIColor[2]));
        }
        else { direct = xyz(load_rgba16f(I.filteredDirect[1], i)); indirect = xyz(load_rgba16f(I.filteredIndirect[1], i)); }
        result = diffuse * (direct + indirect);
        result = lerp3(diffuse, result, d.w);
        if (!LEAN) {
            result = result + xyz(load_rgba16f(I.reflection, i));
            result = result + xyz(load_rgba16f(I.refraction, i));
            result = result + xyz(load_rgba16f(I.transparent, i));
        }
    }
    else result = xyz(d);
    reinterpret_cast<float4 *>(I.output)[i] = make_float4(result.x, result.y, result.z, 1.0f);
    if (!P.separatePost && writeFinal) store_rgba8(I.final, i, result.x, result.y, result.z, 1.0f);   // PostProcessPS passthrough (motionBlurStrength == 0, render size == screen size)
}

// Longest-first order of the one-kernel frame's tiles (device option tile_order; scenes that walk from HBM): tiles sorted by the cost the frame just recorded, most
// expensive first -- a counting sort over min(cost, 1023) in one workgroup (a 1080p frame has 8 160 tiles) -- and the costs cleared for the next frame.  Ties land in
// whatever order the atomics resolve: any permutation renders the same picture.
__global__ __launch_bounds__(1024) void tile_order_kernel(uint32_t *cost, uint32_t *order, uint32_t n) {
    __shared__ uint32_t bucket[1024];
    bucket[threadIdx.x] = 0;
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n; i += 1024) atomicAdd(&bucket[1023u - min(cost[i], 1023u)], 1u);
    __syncthreads();
    // exclusive scan of the 1024 counts: a wave scans its 64, then the 16 wave totals are added up by every thread
    const uint32_t mine = bucket[threadIdx.x];
    uint32_t incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const uint32_t up = (uint32_t)__shfl_up((int)incl, d, 64); if ((threadIdx.x & 63u) >= (uint32_t)d) incl += up; }
    __shared__ uint32_t waveTotal[16];
    if ((threadIdx.x & 63u) == 63u) waveTotal[threadIdx.x >> 6] = incl;
    __syncthreads();
    uint32_t base = 0;
    for (uint32_t w = 0; w < (threadIdx.x >> 6); w++) base += waveTotal[w];
    bucket[threadIdx.x] = base + incl - mine;
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n; i += 1024) {
        const uint32_t b = 1023u - min(cost[i], 1023u);
        order[atomicAdd(&bucket[b], 1u)] = i;
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n; i += 1024) cost[i] = 0;
}

// Extension primary_spp (rule P3, oracle/oracle_render.c): rtOutput of sub-frame `sub` added to the running sum of the frame's sub-frames, in order; the last
// sub-frame turns the sum into the mean (one multiplication by 1.0f / count), stores it as rtOutput and its PostProcessPS passthrough as the back buffer.
__global__ __launch_bounds__(256) void spp_accumulate_kernel(FrameParams Pv, ViewImages Iv, float4 *sum, int sub, int count) {
    PRef P = *kernel_params(); IRef I = *kernel_images(); (void)Pv; (void)Iv; (void)I;
    const int x = blockIdx.x * 32 + (threadIdx.x & 31), y = P.tileY0 + blockIdx.y * 8 + (threadIdx.x >> 5);
    if (x >= P.width || y >= P.tileY1 || !row_owned(P, y)) return;
    const size_t i = (size_t)y * (size_t)P.width + x;
    float4 v = reinterpret_cast<const float4 *>(I.output)[i];
    if (sub > 0) { const float4 a = sum[i]; v.x = a.x + v.x; v.y = a.y + v.y; v.z = a.z + v.z; v.w = a.w + v.w; }
    if (sub + 1 < count) { sum[i] = v; return; }
    const float inv = 1.0f / (float)count;
    v.x *= inv; v.y *= inv; v.z *= inv; v.w *= inv;
    reinterpret_cast<float4 *>(I.output)[i] = v;
    store_rgba8(I.final, i, v.x, v.y, v.z, 1.0f);
}

// PostProcessPS.hlsl:13-36 as its own pass: the screen-size back buffer resampled from the render-size output with the static
// sampler of rt64_device.cpp:958-973 (MIN_MAG_MIP_LINEAR, WRAP), plus the motion-blur gather along gFlow.  Only launched when
// the render size differs from the screen size (RT64_VIEW_DESC.resolutionScale) or motionBlurStrength > 0.
DEV int wrapi(int i, int n) { int j = i % n; return j < 0 ? j + n : j; }
DEV f4 sample_output_linear_wrap(const float *img, int w, int h, float u, float v) {
    const float x = u * (float)w - 0.5f, y = v * (float)h - 0.5f;
    const float x0f = floorf(x), y0f = floorf(y), fx = x - x0f, fy = y - y0f;
    const int x0 = wrapi((int)x0f, w), x1 = wrapi((int)x0f + 1, w), y0 = wrapi((int)y0f, h), y1 = wrapi((int)y0f + 1, h);
    const float4 c00 = reinterpret_cast<const float4 *>(img)[(size_t)y0 * w + x0], c10 = reinterpret_cast<const float4 *>(img)[(size_t)y0 * w + x1];
    const float4 c01 = reinterpret_cast<const float4 *>(img)[(size_t)y1 * w + x0], c11 = reinterpret_cast<const float4 *>(img)[(size_t)y1 * w + x1];
    f4 r;
    { const float top = c00.x + fx * (c10.x - c00.x), bot = c01.x + fx * (c11.x - c01.x); r.x = top + fy * (bot - top); }
    { const float top = c00.y + fx * (c10.y - c00.y), bot = c01.y + fx * (c11.y - c01.y); r.y = top + fy * (bot - top); }
    { const float top = c00.z + fx * (c10.z - c00.z), bot = c01.z + fx * (c11.z - c01.z); r.z = top + fy * (bot - top); }
    r.w = 1.0f;
    return r;
}
DEV f2 sample_flow_linear_wrap(const uint16_t *img, int w, int h, float u, float v) {
    const float x = u * (float)w - 0.5f, y = v * (float)h - 0.5f;
    const float x0f = floorf(x), y0f = floorf(y), fx = x - x0f, fy = y - y0f;
    const int x0 = wrapi((int)x0f, w), x1 = wrapi((int)x0f + 1, w), y0 = wrapi((int)y0f, h), y1 = wrapi((int)y0f + 1, h);
    auto ld = [&](int xx, int yy) { const uint32_t p = reinterpret_cast<const uint32_t *>(img)[(size_t)yy * w + xx]; f2 r; r.x = f16_bits_to_f32((uint16_t)(p & 0xFFFFu)); r.y = f16_bits_to_f32((uint16_t)(p >> 16)); return r; };
    const f2 c00 = ld(x0, y0), c10 = ld(x1, y0), c01 = ld(x0, y1), c11 = ld(x1, y1);
    f2 r;
    { const float top = c00.x + fx * (c10.x - c00.x), bot = c01.x + fx * (c11.x - c01.x); r.x = top + fy * (bot - top); }
    { const float top = c00.y + fx * (c10.y - c00.y), bot = c01.y + fx * (c11.y - c01.y); r.y = top + fy * (bot - top); }
    return r;
}
// Viewport + scissor of the full-screen triangle: the screen, or the rectangles of the first ray-traced instance (rt64_view.cpp:1258-1271,1624-1626).
// False: pixel (x, y) of the back buffer is outside them; otherwise (u, v) is the FullScreenVS interpolant at the pixel centre.
DEV bool full_screen_uv(PRef P, int x, int y, float &u, float &v) {
    const float cx = (float)x + 0.5f, cy = (float)y + 0.5f;
    if (x < P.rtScissor[0] || x >= P.rtScissor[2] || y < P.rtScissor[1] || y >= P.rtScissor[3]) return false;
    if (!(cx >= P.rtViewport[0]) || !(cx < P.rtViewport[0] + P.rtViewport[2]) || !(cy >= P.rtViewport[1]) || !(cy < P.rtViewport[1] + P.rtViewport[3])) return false;
    u = (cx - P.rtViewport[0]) / P.rtViewport[2]; v = (cy - P.rtViewport[1]) / P.rtViewport[3];
    return true;
}
__global__ __launch_bounds__(256) void post_process_kernel(FrameParams Pv, ViewImages Iv) {
    PRef P = *kernel_params(); IRef I = *kernel_images(); (void)Pv; (void)Iv; (void)I;
    const int sw = (int)P.resolution[2], sh = (int)P.resolution[3];
    const int x = blockIdx.x * 32 + (threadIdx.x & 31), y = blockIdx.y * 8 + (threadIdx.x >> 5);
    if (x >= sw || y >= sh) return;
    float u, v;
    if (!full_screen_uv(P, x, y, u, v)) return;
    f4 color; bool blurred = false;
    if (P.motionBlurStrength > 0.0f && P.motionBlurSamples > 0) {
        const f2 fl = sample_flow_linear_wrap(I.flow, P.width, P.height, u, v);
        const float flx = fl.x / P.resolution[0], fly = fl.y / P.resolution[1];
        const float flowLength = sqrtf(flx * flx + fly * fly);
        if (flowLength > 1e-6f) {
            const float sampleStep = P.motionBlurStrength / (float)P.motionBlurSamples;
            float sr = 0.0f, sg = 0.0f, sb = 0.0f, sumWeight = 0.0f;
            const float su = u - (flx * P.motionBlurStrength / 2.0f), sv = v - (fly * P.motionBlurStrength / 2.0f);
            for (uint32_t k = 0; k < P.motionBlurSamples; k++) {
                float uu = su + flx * (float)k * sampleStep, vv = sv + fly * (float)k * sampleStep;
                uu = fminf(fmaxf(uu, 0.0f), 1.0f); vv = fminf(fmaxf(vv, 0.0f), 1.0f);
                const f4 c = sample_output_linear_wrap(P.postSource, P.postSourceW, P.postSourceH, uu, vv);
                sr += c.x * 1.0f; sg += c.y * 1.0f; sb += c.z * 1.0f; sumWeight += 1.0f;
            }
            color = mk4(sr / sumWeight, sg / sumWeight, sb / sumWeight, 1.0f);
            blurred = true;
        }
    }
    if (!blurred) color = sample_output_linear_wrap(P.postSource, P.postSourceW, P.postSourceH, u, v);
    store_rgba8(I.final, (size_t)y * (size_t)sw + x, color.x, color.y, color.z, 1.0f);
}

// One pixel of the debug view's image in its storage format (DebugSource::kind / srcBytes); single-channel images in .x, 32-bit words as their bits.
DEV f4 debug_load(const DebugSource &src, size_t i) {
    if (src.kind == 1) {
        if (src.srcBytes == 8) return load_rgba16f(static_cast<const uint16_t *>(src.ptr), i);
        const uint32_t h = static_cast<const uint32_t *>(src.ptr)[i];                                    // RG16F (flow)
        return mk4(f16_bits_to_f32((uint16_t)(h & 0xFFFFu)), f16_bits_to_f32((uint16_t)(h >> 16)), 0.0f, 0.0f);
    }
    if (src.kind == 2) {
        if (src.srcBytes == 4) return load_rgba8(static_cast<const uint8_t *>(src.ptr), i);
        return mk4(from_unorm8(static_cast<const uint8_t *>(src.ptr)[i]), 0.0f, 0.0f, 0.0f);               // R8 masks
    }
    if (src.srcBytes == 16) { const float4 p = static_cast<const float4 *>(src.ptr)[i]; return mk4(p.x, p.y, p.z, p.w); }
    return mk4(__uint_as_float(static_cast<const uint32_t *>(src.ptr)[i]), 0.0f, 0.0f, 0.0f);           // instance id / depth
}
// DebugPS.hlsl:47-157 in PostProcess's place (device option visualization_mode; rt64_view.cpp:1628-1650): the texel uint2(uv * resolution.xy) of the image the mode
// names -- nearest, zeros out of range -- shown as DebugPS shows it and blended over the back buffer the background pass left (alphaBlendDesc, rt64_device.cpp:532-538:
// SRC_ALPHA / INV_SRC_ALPHA, alpha ONE / INV_SRC_ALPHA, the source clamped to [0, 1] like a UNORM target clamps it).  The mode is uniform over the launch.
__global__ __launch_bounds__(256) void debug_view_kernel(FrameParams Pv, ViewImages Iv, DebugSource src) {
    PRef P = *kernel_params(); IRef I = *kernel_images(); (void)Pv; (void)Iv;
    const int sw = (int)P.resolution[2], sh = (int)P.resolution[3];
    const int x = blockIdx.x * 32 + (threadIdx.x & 31), y = blockIdx.y * 8 + (threadIdx.x >> 5);
    if (x >= sw || y >= sh) return;
    if (!P.separatePost && (y < P.tileY0 || y >= P.tileY1 || !row_owned(P, y))) return;     // back-buffer rows are render rows: this device's only
    float u, v;
    if (!full_screen_uv(P, x, y, u, v)) return;
    const float px = u * P.resolution[0], py = v * P.resolution[1];
    const uint32_t w = (uint32_t)P.width, h = (uint32_t)P.height;
    auto texel = [&](uint32_t tx, uint32_t ty) { return tx < w && ty < h ? debug_load(src, (size_t)ty * w + tx) : mk4(0.0f, 0.0f, 0.0f, 0.0f); };
    f4 c;
    if (src.mode == RT64_IMAGE_FLOW) {
        // getMotionVector: a 1-pixel line from the centre of the pixel's 32 x 32 block along the flow found there (distanceFromLineSegment < 1)
        const float sx = floorf(px / 32.0f) * 32.0f + 16.0f, sy = floorf(py / 32.0f) * 32.0f + 16.0f;
        const f4 fl = texel((uint32_t)rintf(sx), (uint32_t)rintf(sy));
        const float ex = sx + fl.x, ey = sy + fl.y;
        const float len = sqrtf((sx - ex) * (sx - ex) + (sy - ey) * (sy - ey)), l2 = len * len;
        float dist;
        if (l2 == 0.0f) dist = sqrtf((px - sx) * (px - sx) + (py - sy) * (py - sy));
        else {
            const float t = fmaxf(0.0f, fminf(1.0f, ((px - sx) * (ex - sx) + (py - sy) * (ey - sy)) / l2));
            const float qx = sx + t * (ex - sx), qy = sy + t * (ey - sy);
            dist = sqrtf((px - qx) * (px - qx) + (py - qy) * (py - qy));
        }
        c = dist < 1.0f ? mk4(1.0f, 1.0f, 1.0f, 1.0f) : mk4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    else {
        const uint32_t tx = (uint32_t)px, ty = (uint32_t)py;
        c = texel(tx, ty);
        // the G-buffer after the reflection passes: their continuation state where they tagged the pixel (apply_reflection_state_kernel, without the write)
        if (src.reflTag && tx < w && ty < h && I.reflTag[(size_t)ty * w + tx] == src.reflTag) {
            const size_t i = (size_t)ty * w + tx;
            const uint4 s0 = I.reflState0[i], s1 = I.reflState1[i];
            if (src.mode == RT64_IMAGE_SHADING_POSITION) c = mk4(__uint_as_float(s0.x), __uint_as_float(s0.y), __uint_as_float(s0.z), 0.0f);
            else if (src.mode == RT64_IMAGE_SHADING_NORMAL) c = unpack_rgba16f_bits(s1.z, s1.w);
            else c.x = __uint_as_float(s0.w);
        }
        switch (src.mode) {
        case RT64_IMAGE_SHADING_NORMAL: c = mk4((c.x + 1.0f) / 2.0f, (c.y + 1.0f) / 2.0f, (c.z + 1.0f) / 2.0f, 1.0f); break;
        case RT64_IMAGE_INSTANCE_ID: {          // getInstanceId: a colour per instance, nothing on a miss
            const int32_t id = (int32_t)__float_as_uint(c.x);
            if (id < 0) { c = mk4(0.0f, 0.0f, 0.0f, 0.0f); break; }
            uint32_t seed = init_rand((uint32_t)id, 0, 16);
            const float r = next_rand(seed), g = next_rand(seed), b = next_rand(seed);
            c = mk4(r, g, b, 1.0f);
            break;
        }
        case RT64_IMAGE_REACTIVE_MASK: case RT64_IMAGE_LOCK_MASK: case RT64_IMAGE_DEPTH: c = mk4(c.x, c.x, c.x, 1.0f); break;
        default: c.w = 1.0f;
        }
    }
    auto unorm = [](float a) { return a > 0.0f ? fminf(a, 1.0f) : 0.0f; };
    const float r = unorm(c.x), g = unorm(c.y), b = unorm(c.z), a = unorm(c.w), ia = 1.0f - a;
    const size_t i = (size_t)y * (size_t)sw + x;
    const f4 d = load_rgba8(I.final, i);
    store_rgba8(I.final, i, r * a + d.x * ia, g * a + d.y * ia, b * a + d.z * ia, a + d.w * ia);
}

// IndirectRayGen with giSamples == 0 (IndirectRayGen.hlsl:135): every pixel gets ambientBase + ambientNoGI, history 0.
__global__ __launch_bounds__(256) void indirect_constant_kernel(FrameParams Pv, ViewImages Iv, int cur) {
    PRef P = *kernel_params(); IRef I = *kernel_images(); (void)Pv; (void)Iv; (void)I;
    const int x = blockIdx.x * 32 + (threadIdx.x & 31), y = P.tileY0 + blockIdx.y * 8 + (threadIdx.x >> 5);
    if (x >= P.width || y >= P.tileY1 || !row_owned(P, y)) return;
    const size_t i = (size_t)y * (size_t)P.width + x;
    const float r = P.ambientBaseColor[0] + P.ambientNoGIColor[0], g = P.ambientBaseColor[1] + P.ambientNoGIColor[1], b = P.ambientBaseColor[2] + P.ambientNoGIColor[2];
    store_rgba16f(I.indirectLight[cur], i, r, g, b, 0.0f);
    store_rgba16f(I.filteredIndirect[1], i, r, g, b, 0.0f);
}

// The reflection passes keep their continuation state beside the G-buffer (ViewImages::reflState0 / 1); the reference rewrites the G-buffer itself
// (ReflectionRayGen.hlsl:117-124).  A reader of gShadingPosition / gViewDirection / gShadingNormal / gInstanceId gets the reference's bytes through this
// kernel: every pixel the frame's passes tagged takes its last state (View::applyReflectionState, on readback only).
__global__ __launch_bounds__(256) void apply_reflection_state_kernel(ViewImages I, int width, int y0, int y1, uint32_t frameTag) {
    const int x = blockIdx.x * 32 + (threadIdx.x & 31), y = y0 + blockIdx.y * 8 + (threadIdx.x >> 5);
    if (x >= width || y >= y1) return;
    const size_t i = (size_t)y * (size_t)width + x;
    if (I.reflTag[i] != frameTag) return;
    const uint4 s0 = I.reflState0[i], s1 = I.reflState1[i];
    reinterpret_cast<float4 *>(I.shadingPosition)[i] = make_float4(__uint_as_float(s0.x), __uint_as_float(s0.y), __uint_as_float(s0.z), 0.0f);
    reinterpret_cast<uint2 *>(I.viewDirection)[i] = make_uint2(s1.x, s1.y);
    reinterpret_cast<uint2 *>(I.shadingNormal)[i] = make_uint2(s1.z, s1.w);
    I.instanceId[i] = (int32_t)s0.w;
}

__global__ __launch_bounds__(256) void clear_final_kernel(FrameParams Pv, ViewImages Iv) {
    PRef P = *kernel_params(); IRef I = *kernel_images(); (void)Pv; (void)Iv; (void)I;
    if (P.separatePost) {         // the back buffer has the screen size, the frame is not partitioned
        const int sw = (int)P.resolution[2], sh = (int)P.resolution[3];
        const int x = blockIdx.x * 32 + (threadIdx.x & 31), y = blockIdx.y * 8 + (threadIdx.x >> 5);
        if (x < sw && y < sh) store_rgba8(I.final, (size_t)y * (size_t)sw + x, 0.0f, 0.0f, 0.0f, 1.0f);
        return;
    }
    const int x = blockIdx.x * 32 + (threadIdx.x & 31), y = P.tileY0 + blockIdx.y * 8 + (threadIdx.x >> 5);
    if (x >= P.width || y >= P.tileY1 || !row_owned(P, y)) return;
    store_rgba8(I.final, (size_t)y * (size_t)P.width + x, 0.0f, 0.0f, 0.0f, 1.0f);   // cleared back buffer, rt64_device.cpp:996-997
}

}  // namespace

// One spill slab per lane of every workgroup of the largest grid a frame of `width` x `rows` can launch: the persistent kernels use
// at most RT_GRID_BLOCKS workgroups, the one-kernel frame one per 16 x 16 tile.
size_t rt_stack_spill_bytes(int width, int rows) {
    const size_t tiles = (size_t)((width + 15) / 16) * (size_t)((rows + 15) / 16);
    size_t blocks = tiles > (size_t)RT_GRID_BLOCKS ? tiles : (size_t)RT_GRID_BLOCKS;
    if (blocks > RT_MAX_FRAME_GROUPS) blocks = RT_MAX_FRAME_GROUPS;
    blocks += 8;          // the per-wave frame rounds its grid up to whole groups of 8 tiles (32 one-wave workgroups)       // no launch has more workgroups than that (launch_lean_frame, sparse_grid)
    return blocks * RT_BLOCK * (RT_STACK_SPILL_HEADER + RT_STACK_SPILL) * sizeof(uint32_t);      // (a lane's entries + the header in front of them: trace.h)
}
// Host side of tile_count: the 16-row strips stripRank, stripRank + stripCount, ... of [tileY0, tileY1) are this device's.
unsigned owned_tiles(const FrameParams &P, bool rowTiles) {
    const unsigned all = (unsigned)(P.tileY1 - P.tileY0 + 15) / 16;
    const unsigned strips = all > (unsigned)P.stripRank ? (all - (unsigned)P.stripRank + (unsigned)P.stripCount - 1) / (unsigned)P.stripCount : 0u;
    return rowTiles ? (unsigned)((P.width + 31) / 32) * strips * 2u : (unsigned)((P.width + 15) / 16) * strips;
}

hipError_t launch_scene_cache_image(const GpuInstance *instances, const uint32_t *tlasIndex, const GpuNode *tlasNodes, uint32_t cacheInstances, void *image, bool blasOnly, hipStream_t s) {
    return launch(scene_cache_image_kernel, 1, RT_BLOCK, 0, s, instances, tlasIndex, tlasNodes, cacheInstances, static_cast<u32x4 *>(image), blasOnly ? 1 : 0);
}
hipError_t launch_primary_trace(const FrameParams &P, const ViewImages &I, int32_t *hitInstance, bool klist, hipStream_t s) {
    if (klist) return launch(primary_trace_kernel<true>, rt_grid(P), RT_BLOCK, 0, s, P, I, hitInstance);
    if (P.cacheWords) return launch(primary_trace_kernel<false, true>, rt_grid(P), RT_BLOCK, cached_lds_bytes(P, false), s, P, I, hitInstance);
    return launch(primary_trace_kernel<false>, rt_grid(P), RT_BLOCK, 0, s, P, I, hitInstance);
}
hipError_t launch_indirect_constant(const FrameParams &P, const ViewImages &I, int cur, hipStream_t s) {
    return launch(indirect_constant_kernel, image_grid(P.width, P.tileY1 - P.tileY0), 256, 0, s, P, I, cur);
}
hipError_t launch_gaussian(const uint16_t *in, uint16_t *out, int width, int height, int y0, int y1, hipStream_t s) {
    return launch(gaussian_kernel, image_grid(width, y1 - y0), 256, 0, s, in, out, width, height, y0, y1);
}
hipError_t launch_compose_post(const FrameParams &P, const ViewImages &I, int cur, bool lean, bool writeFinal, hipStream_t s) {
    return with_flag(lean, [&](auto LEAN) { return launch(compose_post_kernel<decltype(LEAN)::value>, image_grid(P.width, P.tileY1 - P.tileY0), 256, 0, s, P, I, cur, writeFinal ? 1 : 0); });
}
hipError_t launch_tile_order(uint32_t *cost, uint32_t *order, uint32_t tiles, hipStream_t s) {
    return launch(tile_order_kernel, 1, 1024, 0, s, cost, order, tiles);
}
hipError_t launch_spp_accumulate(const FrameParams &P, const ViewImages &I, float *sum, int sub, int count, hipStream_t s) {
    return launch(spp_accumulate_kernel, image_grid(P.width, P.tileY1 - P.tileY0), 256, 0, s, P, I, reinterpret_cast<float4 *>(sum), sub, count);
}
hipError_t launch_post_process(const FrameParams &P, const ViewImages &I, hipStream_t s) {
    return launch(post_process_kernel, image_grid((int)P.resolution[2], (int)P.resolution[3]), 256, 0, s, P, I);
}
hipError_t launch_debug_view(const FrameParams &P, const ViewImages &I, const DebugSource &src, hipStream_t s) {
    return launch(debug_view_kernel, image_grid((int)P.resolution[2], (int)P.resolution[3]), 256, 0, s, P, I, src);
}
__global__ __launch_bounds__(256) void stack_slab_init_kernel(uint32_t *slab, size_t lanes, const uint32_t *flag) {
    const size_t lane = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (lane >= lanes) return;
    const uint64_t p = reinterpret_cast<uint64_t>(flag);
    uint32_t *h = slab + lane * (RT_STACK_SPILL_HEADER + RT_STACK_SPILL);
    h[0] = (uint32_t)p; h[1] = (uint32_t)(p >> 32);
}
hipError_t launch_stack_slab_init(uint32_t *slab, size_t lanes, const uint32_t *flagDevicePointer, hipStream_t s) {
    if (!lanes) return hipSuccess;
    return launch(stack_slab_init_kernel, (unsigned)((lanes + 255) / 256), 256, 0, s, slab, lanes, flagDevicePointer);
}
hipError_t launch_apply_reflection_state(const ViewImages &I, int width, int y0, int y1, uint32_t frameTag, hipStream_t s) {
    if (y1 <= y0) return hipSuccess;
    return launch(apply_reflection_state_kernel, image_grid(width, y1 - y0), 256, 0, s, I, width, y0, y1, frameTag);
}
hipError_t launch_clear_final(const FrameParams &P, const ViewImages &I, hipStream_t s) {
    const dim3 grid = P.separatePost ? image_grid((int)P.resolution[2], (int)P.resolution[3]) : image_grid(P.width, P.tileY1 - P.tileY0);
    return launch(clear_final_kernel, grid, 256, 0, s, P, I);
}
