// pass_common.h -- what the two translation units of the frame's passes share: passes.hip (the ray kernels that exist twice, general and
// "simple") and image_passes.hip (the kernels that are compiled once).  Device side: the pixel tiles a workgroup walks, the per-lane
// traversal resources of a ray kernel (LDS stack, scene cache, light-candidate columns) and the surface ray.  Host side: the launch shapes.
#pragma once
#include <type_traits>
#include "kernels.h"
#include "shade.h"

struct Pixel { uint32_t x, y; bool valid; };

// Pixel tiles.  A workgroup (4 waves) owns one tile per loop trip; two shapes:
//   SQUARE 16x16, wave = 8x8 pixels   : traversal kernels (coherent rays share BVH nodes)
//   ROWS   32x8,  wave = 32x2 pixels  : shading kernels (a wave's image store covers whole 128/256-byte lines)
// Tile rows owned by this device: strips stripRank, stripRank + stripCount, ... of the 16-row strips in [tileY0, tileY1).
enum TileShape { TILE_SQUARE = 0, TILE_ROWS = 1 };
template <int SHAPE> struct TileDim { static constexpr int W = SHAPE == TILE_SQUARE ? 16 : 32, H = SHAPE == TILE_SQUARE ? 16 : 8; };

DEV uint32_t owned_strips(PRef P) {
    const uint32_t all = (uint32_t)(P.tileY1 - P.tileY0 + 15) / 16;
    return all > (uint32_t)P.stripRank ? (all - (uint32_t)P.stripRank + (uint32_t)P.stripCount - 1) / (uint32_t)P.stripCount : 0u;
}
template <int SHAPE = TILE_SQUARE> DEV uint32_t tile_count(PRef P) {
    return (uint32_t)((P.width + TileDim<SHAPE>::W - 1) / TileDim<SHAPE>::W) * owned_strips(P) * (16u / TileDim<SHAPE>::H);
}
template <int SHAPE = TILE_SQUARE> DEV Pixel tile_pixel_at(PRef P, uint32_t tile, uint32_t wave, uint32_t lane) {
    constexpr uint32_t TW = TileDim<SHAPE>::W, TH = TileDim<SHAPE>::H, perStrip = 16u / TH;
    const uint32_t tilesX = ((uint32_t)P.width + TW - 1) / TW;
    const uint32_t tx = tile % tilesX, lt = tile / tilesX;
    const uint32_t strip = (lt / perStrip) * (uint32_t)P.stripCount + (uint32_t)P.stripRank;
    Pixel p;
    if (SHAPE == TILE_SQUARE) { p.x = tx * TW + (wave & 1) * 8 + (lane & 7); p.y = (wave >> 1) * 8 + (lane >> 3); }
    else { p.x = tx * TW + (lane & 31); p.y = wave * 2 + (lane >> 5); }
    p.y += (uint32_t)P.tileY0 + strip * 16 + (lt % perStrip) * TH;
    p.valid = p.x < (uint32_t)P.width && p.y < (uint32_t)P.tileY1;
    return p;
}
template <int SHAPE = TILE_SQUARE> DEV Pixel tile_pixel(PRef P, uint32_t tile) {
    return tile_pixel_at<SHAPE>(P, tile, threadIdx.x >> 6, threadIdx.x & 63);
}

DEV bool row_owned(PRef P, int y) { return (((y - P.tileY0) / 16) % P.stripCount) == P.stripRank; }

// uint32 words of a kernel's LDS stack array per lane: RT_STACK_LDS entries, or RT_STACK_LDS_CACHED int16 entries in the kernels that hold the scene cache
constexpr uint32_t stack_words(bool cached) { return cached ? RT_STACK_LDS_CACHED / 2 : RT_STACK_LDS; }
DEV TraceStack make_stack(PRef P, uint32_t *ldsStack, uint32_t wordsPerLane) {
    TraceStack s;
    uint32_t *block = ldsStack + (threadIdx.x >> 6) * wordsPerLane * RT_LANES;       // this wave's [entry][lane] block
    s.lds = (LdsU32Ptr)(block + (threadIdx.x & 63u));
    s.lds16 = (LdsI16Ptr)block + (threadIdx.x & 63u);
    s.spill = (GlobalU32Ptr)(P.traversalStack + ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * (RT_STACK_SPILL_HEADER + RT_STACK_SPILL) + RT_STACK_SPILL_HEADER);
    s.cache = nullptr; s.ldsEntries = RT_STACK_LDS;
    return s;
}
// this lane's columns of the light-candidate arrays, [wave][slots][lane] (floats, then bytes)
DEV void light_columns(ShadeEnv &env, float *intensities, uint8_t *indices, uint32_t slots) {
    const uint32_t at = (threadIdx.x >> 6) * slots * RT_LANES + (threadIdx.x & 63u);
    env.lightIntensity = intensities + at; env.lightIndex = indices + at;
}

// CACHED variants of the ray kernels keep the scene cache and the light-selection columns in dynamic LDS:
//   [scene cache: P.cacheWords x 16 B][light intensities: slots x RT_BLOCK floats][light indices: slots x RT_BLOCK bytes], slots = min(lights, 16) + 1
DEV uint32_t light_slots(PRef P) { return (P.lightCount < RT64_MAX_LIGHTS ? P.lightCount : (uint32_t)RT64_MAX_LIGHTS) + 1u; }

// The scene cache is filled once per workgroup by fill_scene_cache (trace.h: its layout, and the one-round-trip copy the query kernels share).

// ---- the prologue of a ray kernel -------------------------------------------------------------------------------------------
// The __shared__ arrays stay declared in the kernels (their sizes depend on the kernel's template arguments, their order is the LDS layout); these two
// hand this lane its share of them.  CACHED: the walk reads nodes from the LDS scene cache at dynLds and keeps int16 stack entries.
// Pure traversal (no light is picked): the caller has filled the scene cache -- the bounce walks do that behind their early exit.
template <bool CACHED> DEV void traversal_env(PRef P, ShadeEnv &env, uint32_t *ldsStack, const u32x4_lds *dynLds) {
    env.stk = make_stack(P, ldsStack, stack_words(CACHED)); env.cnt = TraceCounts(); env.shadowRays = 0;
    env.lightIntensity = nullptr; env.lightIndex = nullptr;
    if (CACHED) env.stk.use_cache(dynLds);
}
// Kernels that pick lights.  The light-candidate columns are the kernel's static arrays of RT64_MAX_LIGHTS + 1 slots, or sit in dynamic LDS sized by the frame's
// light count: behind the scene cache of a CACHED kernel -- [scene cache: P.cacheWords x 16 B][light intensities: slots x block floats][light indices: slots x block
// bytes], slots = light_slots(P); the cache is filled here (all threads call this; ends with a barrier) -- and at dynLds itself in the one-kernel frame without the
// cache (STATIC_COLUMNS = false: it declares no static arrays; BLOCK threads).
template <bool CACHED, bool STATIC_COLUMNS = true, int BLOCK = RT_BLOCK>
DEV void shading_env(PRef P, ShadeEnv &env, uint32_t *ldsStack, float *ldsLightIntensity, uint8_t *ldsLightIndex, u32x4_lds *dynLds) {
    env.stk = make_stack(P, ldsStack, stack_words(CACHED)); env.cnt = TraceCounts(); env.shadowRays = 0;
    if (STATIC_COLUMNS) light_columns(env, ldsLightIntensity, ldsLightIndex, RT64_MAX_LIGHTS + 1);
    if (STATIC_COLUMNS && !CACHED) return;
    if (CACHED) { fill_scene_cache(P, dynLds); env.stk.use_cache(dynLds); }
    float *li = reinterpret_cast<float *>(dynLds + (CACHED ? P.cacheWords : 0u));
    light_columns(env, li, reinterpret_cast<uint8_t *>(li + light_slots(P) * (CACHED ? blockDim.x : (uint32_t)BLOCK)), light_slots(P));
}

DEV void flush_env(PRef P, const ShadeEnv &env, int pass, int rayCounter, uint32_t rays) {
    flush_counts(P, env.cnt, pass);
    if (!P.countTraversal) return;
    unsigned long long a = rays, b = env.shadowRays;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { a += __shfl_down(a, d, 64); b += __shfl_down(b, d, 64); }
    if ((threadIdx.x & 63) == 0) { unsigned long long *ctr = P.counters + (size_t)(blockIdx.x % RT_COUNTER_STRIPES) * CTR_COUNT; if (a) atomicAdd(&ctr[rayCounter], a); if (b) atomicAdd(&ctr[CTR_SHADOW], b); }
}

// ---- surface rays ---------------------------------------------------------------------------------------------------------
// Sort key = t - depthBias (WithDistanceBias, Instances.hlsli:17-19); ties keep the first-come hit like the reference's
// strict '<' insertion (rt64_shader.cpp:557).  Hits on instances flagged opaque (rule O1) shorten tmax (R5):
// lim = (t - depthBias) + maxDepthBias.
//   KLIST = false: every instance of the frame is provably opaque -> the list degenerates to the closest hit (registers).
//   KLIST = true : sorted insertion into the per-pixel list in HBM, 16 entries + 1 scratch slot, exactly the any-hit of
//                  rt64_shader.cpp:547-581 (a hit that lands in slot 15 commits tmax; nhits keeps counting).
struct SurfaceHit { float key, t, u, v; uint32_t instance, prim; bool hit; };

template <bool KLIST, bool CACHED = false>
DEV uint32_t trace_surface(PRef P, ShadeEnv &env, IRef I, size_t pixel, f3 o, f3 d, const RayDiff &rayDiff,
                           uint32_t px, uint32_t py, SurfaceHit &best) {
    float oo[3] = { o.x, o.y, o.z }, dd[3] = { d.x, d.y, d.z };
    best.hit = false; best.key = INFINITY;
    uint32_t nhits = 0;
    const size_t stride = (size_t)P.width * (size_t)P.height;
    trace_ray<CACHED>(P, oo, dd, RT_RAY_MIN_DISTANCE, RT_RAY_MAX_DISTANCE, true, env.stk,
              [&](float t, float u, float v, uint32_t instance, uint32_t prim, float &tmax, uint32_t instFlags, float instDepthBias) -> bool {
                  const GpuInstance &in = P.instances[instance];
                  const float key = t - instDepthBias;
                  if (!KLIST) {
                      if (key < best.key) { best.key = key; best.t = t; best.u = u; best.v = v; best.instance = instance; best.prim = prim; best.hit = true; }
                  }
                  else {
                      if (in.cc.optTextureEdge) {            // IgnoreHit() before the hit is stored (rt64_shader.cpp:502-511)
                          HitRecord tmp;
                          if (!surface_anyhit(P, instance, prim, t, u, v, d, rayDiff, px, py, tmp)) return false;
                      }
                      uint32_t hi = nhits < RT64_MAX_HIT_QUERIES ? nhits : RT64_MAX_HIT_QUERIES;
                      while (hi > 0) {
                          const uint4 prev = I.klistA[(size_t)(hi - 1) * stride + pixel];
                          if (!(key < __uint_as_float(prev.x))) break;
                          I.klistA[(size_t)hi * stride + pixel] = prev;
                          I.klistB[(size_t)hi * stride + pixel] = I.klistB[(size_t)(hi - 1) * stride + pixel];
                          hi--;
                      }
                      if (hi < RT64_MAX_HIT_QUERIES) {
                          I.klistA[(size_t)hi * stride + pixel] = make_uint4(__float_as_uint(key), __float_as_uint(u), __float_as_uint(v), prim);
                          I.klistB[(size_t)hi * stride + pixel] = make_uint2(__float_as_uint(t), instance);
                          ++nhits;
                          if (hi == RT64_MAX_HIT_QUERIES - 1 && t < tmax) tmax = t;      // not IgnoreHit(): the hit is committed
                      }
                      if (!(instFlags & GPU_INST_OPAQUE)) return false;
                  }
                  const float lim = key + P.maxDepthBias;
                  if (lim < tmax) tmax = lim;
                  return false;
              }, env.cnt);
    return KLIST ? nhits : (best.hit ? 1u : 0u);
}

constexpr int TRACE_WAVES = 4;         // waves/SIMD the register allocator must fit for pure-traversal kernels (5 spills, measured no faster)
// ---- launch shapes (host) ---------------------------------------------------------------------------------------------------
// Grid of a ray kernel: one persistent workgroup per CU slot (RT_GRID_BLOCKS), or one per tile when the device's share of the
// frame has fewer tiles than that (small frames, a 1/8 strip share): workgroups without a tile only cost launch time.
static unsigned rt_grid(const FrameParams &P) {
    const unsigned tiles = owned_tiles(P, true);          // (never fewer than the 16 x 16 tiles: two 32 x 8 tiles per 32 columns of a strip)
    return tiles < 1u ? 1u : (tiles < (unsigned)RT_GRID_BLOCKS ? tiles : (unsigned)RT_GRID_BLOCKS);
}
// dynamic LDS of a CACHED kernel: scene cache, plus the light-selection columns when the kernel picks lights
static size_t cached_lds_bytes(const FrameParams &P, bool lights) {
    const size_t slots = (P.lightCount < RT64_MAX_LIGHTS ? P.lightCount : (uint32_t)RT64_MAX_LIGHTS) + 1u;
    return (size_t)P.cacheWords * 16 + (lights ? (slots * RT_BLOCK * 5 + 15) / 16 * 16 : 0);
}
// Grid of an image-space kernel over w x rows pixels: workgroups of 256 threads, 32 x 8 pixels each.
static inline dim3 image_grid(int w, int rows) { return dim3((unsigned)(w + 31) / 32, (unsigned)(rows + 7) / 8); }
template <class... Params, class... Args>
static inline void enqueue(void (*kernel)(Params...), dim3 grid, unsigned block, size_t ldsBytes, hipStream_t s, const Args &... args) {
    hipLaunchKernelGGL(kernel, grid, dim3(block), ldsBytes, s, args...);
}
template <class... Params, class... Args>
static inline hipError_t launch(void (*kernel)(Params...), dim3 grid, unsigned block, size_t ldsBytes, hipStream_t s, const Args &... args) {
    enqueue(kernel, grid, block, ldsBytes, s, args...);
    return hipGetLastError();
}
// A runtime flag as a template argument: f(std::true_type) or f(std::false_type); the launchers nest it once per flag of the kernel.
template <class F> static inline auto with_flag(bool flag, F &&f) { return flag ? f(std::true_type()) : f(std::false_type()); }
