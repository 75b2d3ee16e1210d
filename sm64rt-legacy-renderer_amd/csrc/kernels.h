// kernels.h -- host-callable launchers of the HIP kernels in librt64.so.
#pragma once
#include <hip/hip_runtime.h>
#include "rt64_gpu.h"
#include "../../include/rt64_lighting.h"     // (includes rt64_alpha.h, rt64_material.h, rt64_surface.h and rt64_query.h)
#include "../../include/rt64_sampled_lighting.h"
#include "../../include/rt64_footprint.h"
#include "../../include/rt64_bounce.h"
#include "../../include/rt64_layers.h"
#include "../../include/rt64_radiance.h"

// ---- lbvh.hip ---------------------------------------------------------------------------------------------------
#define LBVH_SMALL_MAX 4096u          // leaves handled by the single-workgroup LDS builder
enum { LBVH_MODE_TRIANGLES = 0, LBVH_MODE_INSTANCES = 1 };

struct LbvhArgs {
    int mode, refit;
    uint32_t n;
    // LBVH_MODE_TRIANGLES
    const uint8_t *vertices; uint32_t vertexStride; const uint32_t *indices;
    // LBVH_MODE_INSTANCES
    const GpuInstance *instances;
    // outputs
    GpuNode *nodes;                   // max(n-1, 1)
    GpuTri *tris;                     // n (triangles mode)
    BlasHeader *header;
    uint32_t *sortedIndex, *morton, *leafParent;   // n each
    // scratch for the large path (allocated by the caller when n > LBVH_SMALL_MAX)
    void *scratch; size_t scratchBytes;
};

size_t lbvh_small_lds_bytes(uint32_t n);
size_t lbvh_large_scratch_bytes(uint32_t n);
hipError_t lbvh_launch(const LbvhArgs &args, hipStream_t stream);
hipError_t lbvh_launch_large(const LbvhArgs &args, hipStream_t stream);
hipError_t lbvh_launch_batch(const LbvhArgs *deviceArgs, uint32_t count, uint32_t maxN, hipStream_t stream);   // one workgroup per tree, n <= LBVH_SMALL_MAX each

// ---- bc7.hip ------------------------------------------------------------------------------------------------------
// Decode `blocksX * blocksY` BC7 blocks into an RGBA8 image of width x height texels.
// RGBA8 image (row-major) -> the same texels in 4 x 4 tiles of 64 bytes (width, height multiples of 4).
hipError_t tile_texture_launch(const uint8_t *rgba, uint32_t *tiled, uint32_t width, uint32_t height, hipStream_t stream);
hipError_t bc7_decode_launch(const uint8_t *blocks, uint8_t *rgba, uint32_t width, uint32_t height, hipStream_t stream);

// ---- bcn.hip ------------------------------------------------------------------------------------------------------
// A DDS chain of BC1-BC5 blocks or BGRA8 / BGRX8 texels -> RGBA8 (rules D1-D7 in bcn.hip), every level in ONE launch.  Level m of the
// source starts where level m - 1 ends (ceil(w / 4) * ceil(h / 4) blocks of bcn_block_bytes(format), or w * h texels); level m of `rgba` at
// mipOffset[m] texels.  BGRA8 / BGRX8 convert in place: pass src == rgba, holding the file's texels.
enum BcnFormat : uint32_t { BCN_BC1 = 1, BCN_BC2, BCN_BC3, BCN_BC4, BCN_BC5, BCN_BGRA8, BCN_BGRX8 };
uint32_t bcn_block_bytes(uint32_t format);           // 8 (BC1, BC4) or 16 (BC2, BC3, BC5)
hipError_t bcn_decode_launch(const uint8_t *src, uint8_t *rgba, uint32_t format, const uint32_t *mipOffset, uint32_t width, uint32_t height, int levels, hipStream_t stream);

// ---- mipgen.hip ---------------------------------------------------------------------------------------------------
// Mip chain of an RGBA8 texture (device option generate_mipmaps; rules M1-M6 in mipgen.hip): level 0 is in place at mipOffset[0], the
// launches make levels 1 .. levels - 1.  A chain whose level 1 holds at most MIPGEN_TAIL_TEXELS texels is one launch of one workgroup.
#define MIPGEN_TAIL_TEXELS 4096u
int mipgen_level_count(int width, int height);       // M2: min(floor(log2(max(w, h))) + 1, RT64_MAX_MIPS)
hipError_t mipgen_launch(uint8_t *texels, const uint32_t *mipOffset, uint32_t width, uint32_t height, int levels, hipStream_t stream);

// ---- passes.hip (the ray kernels that also exist as `_simple` twins) + image_passes.hip (everything compiled once) ----
#define RT_CACHE_MAX_WORDS 1536       // LDS scene cache, nodes + instance records: at most 24 KB next to the 8 KB stack (int16 entries) and the light columns of a workgroup, four workgroups per CU
#define RT_STACK_LDS 24               // traversal stack entries per lane in LDS of the kernels without the scene cache; deeper levels go to the HBM spill slab
#define RT_STACK_LDS_CACHED 16        // traversal stack entries of the kernels that hold the LDS scene cache: the host enables the cache only when TLAS depth + the deepest
                                      // BLAS fit in these entries (BlasHeader::depth), so their push / pop are plain LDS accesses -- no spill branch in the node loop; a power of two
#define RT_STACK_SPILL 84             // entries per lane in the HBM slab behind the LDS entries
#define RT_STACK_SPILL_HEADER 2       // uint32 words in front of EVERY lane's entries: the address of the overflow word (host-pinned memory); a lane's slab is RT_STACK_SPILL_HEADER + RT_STACK_SPILL words
hipError_t launch_stack_slab_init(uint32_t *slab, size_t lanes, const uint32_t *flagDevicePointer, hipStream_t s);      // writes every lane's header
#define RT_GRID_BLOCKS 2048           // persistent grid of every ray kernel (8 workgroups of 256 per CU)
#define RT_TIMING_WAVES ((8192u + 8u) * 4u)   // waves the tile-timing buffer has records for (profiling aid)
#define RT_MAX_BOUNCE_GROUPS 65536u    // largest grid of the bounce kernels (one workgroup per 16 x 16 tile up to 4K and beyond; hit-list segments and counts are sized for it)
#define RT_MAX_FRAME_GROUPS 8192u     // largest grid of the one-workgroup-per-tile kernels (bigger frames give every workgroup a few tiles)
size_t rt_stack_spill_bytes(int width, int rows);        // bytes FrameParams::traversalStack needs for a frame of that size

hipError_t launch_scene_cache_image(const GpuInstance *instances, const uint32_t *tlasIndex, const GpuNode *tlasNodes, uint32_t cacheInstances, void *image, bool blasOnly, hipStream_t s);   // LDS scene cache contents, flat (FrameParams::cacheImage)
hipError_t launch_primary_trace(const FrameParams &P, const ViewImages &I, int32_t *hitInstance, bool klist, hipStream_t s);
hipError_t launch_primary_shade(const FrameParams &P, const ViewImages &I, const int32_t *hitInstance, int cur, bool transparentLighting, bool lean, hipStream_t s);
hipError_t launch_direct(const FrameParams &P, const ViewImages &I, int cur, bool lean, hipStream_t s);
enum { BOUNCE_WALK_PLAIN = 0, BOUNCE_WALK_REFILL = 1, BOUNCE_WALK_SPLIT = 2 };      // how bounce_trace hands rays to lanes (passes.hip)
// walk: how bounce_trace hands rays to lanes; groups: grid of the bounce kernels (0 = the persistent grid)
hipError_t launch_indirect(const FrameParams &P, const ViewImages &I, int cur, bool writeFiltered, bool klist, int walk, unsigned groups, int writeGuide, hipStream_t s);      // writeGuide: bounce_resolve_kernel also writes the SVGF guide records of its rows (wavefront chain only: !klist, bounce records allocated)
hipError_t launch_indirect_constant(const FrameParams &P, const ViewImages &I, int cur, hipStream_t s);
hipError_t launch_refraction(const FrameParams &P, const ViewImages &I, bool klist, hipStream_t s);
hipError_t launch_reflection(const FrameParams &P, const ViewImages &I, bool klist, int pass, bool last, int parity, hipStream_t s);      // pass / last / parity: see reflection_kernel (ViewImages::reflectFlags)
hipError_t launch_gaussian(const uint16_t *in, uint16_t *out, int width, int height, int y0, int y1, hipStream_t s);
hipError_t launch_compose_post(const FrameParams &P, const ViewImages &I, int cur, bool lean, bool writeFinal, hipStream_t s);
// A lean frame in one launch: primary visibility + resolve + direct light + compose (passes.hip, lean_frame_kernel).
// Frames without the LDS scene cache run one wave (an 8 x 8 wave-tile) per workgroup, frames with it one 16 x 16 tile per workgroup.
// maxGroups: cap of the grid (RT_MAX_FRAME_GROUPS; device option max_frame_groups lowers it so that small frames exercise the several-tiles-per-workgroup walk)
hipError_t launch_lean_frame(const FrameParams &P, const ViewImages &I, int32_t *hitInstance, int cur, bool full, int ownedY0, int ownedY1, unsigned maxGroups, hipStream_t s);
hipError_t launch_post_process(const FrameParams &P, const ViewImages &I, hipStream_t s);      // PostProcessPS as its own pass (resolution scale / motion blur)
// DebugPS in PostProcess's place (device option visualization_mode): the image the view shows, as RT64_ReadbackDevice selects it -- its storage
// (kind: 0 raw 32-bit words, 1 half floats, 2 unorm8; srcBytes per pixel) and, for modes 1, 2 and 5, the frame tag of the reflection passes' state
// (ViewImages::reflTag; 0: none) that a readback would fold back into the G-buffer first
struct DebugSource { const void *ptr; int srcBytes, kind, mode; uint32_t reflTag; };
hipError_t launch_debug_view(const FrameParams &P, const ViewImages &I, const DebugSource &src, hipStream_t s);
// passes_simple.hip: the same launchers over kernels compiled without non-power-of-two texture addressing and without the shadow any-hit
// program; the launchers above route to them when FrameParams::simpleKernels is set
hipError_t launch_primary_shade_simple(const FrameParams &P, const ViewImages &I, const int32_t *hitInstance, int cur, bool transparentLighting, bool lean, hipStream_t s);
hipError_t launch_direct_simple(const FrameParams &P, const ViewImages &I, int cur, bool lean, hipStream_t s);
hipError_t launch_indirect_simple(const FrameParams &P, const ViewImages &I, int cur, bool writeFiltered, bool klist, int walk, unsigned groups, int writeGuide, hipStream_t s);
hipError_t launch_refraction_simple(const FrameParams &P, const ViewImages &I, bool klist, hipStream_t s);
hipError_t launch_reflection_simple(const FrameParams &P, const ViewImages &I, bool klist, int pass, bool last, int parity, hipStream_t s);
hipError_t launch_lean_frame_simple(const FrameParams &P, const ViewImages &I, int32_t *hitInstance, int cur, bool full, int ownedY0, int ownedY1, unsigned maxGroups, hipStream_t s);
hipError_t launch_clear_final(const FrameParams &P, const ViewImages &I, hipStream_t s);
hipError_t launch_apply_reflection_state(const ViewImages &I, int width, int y0, int y1, uint32_t frameTag, hipStream_t s);      // rows [y0, y1): the continuation state the reflection passes tagged `frameTag` folded back into the G-buffer (readback only)
unsigned owned_tiles(const FrameParams &P, bool rowTiles = false);     // 16 x 16 tiles (rowTiles: 32 x 8) of the rows this device owns: the host's count of what tile_count walks
hipError_t launch_tile_order(uint32_t *cost, uint32_t *order, uint32_t tiles, hipStream_t s);
hipError_t launch_spp_accumulate(const FrameParams &P, const ViewImages &I, float *sum, int sub, int count, hipStream_t s);

// ---- query.hip -----------------------------------------------------------------------------------------------------
// RT64_TraceViewRays: `count` RT64_RAYs -> RT64_RAY_HITs (device pointers, 16-byte aligned) against the tables of P (the view's last frame; rules Q1-Q7).
// P.traversalStack: a slab of ray_query_spill_bytes() with its lane headers written, or nullptr when no walk of the scene outgrows the LDS stack.
size_t ray_query_spill_bytes();
hipError_t launch_ray_query(const FrameParams &P, const void *rays, void *hits, uint64_t count, uint32_t flags, hipStream_t s);

// ---- surface.hip ---------------------------------------------------------------------------------------------------
// RT64_ResolveViewRayHits: `count` RT64_RAYs and their RT64_RAY_HITs -> RT64_RAY_SURFACEs (device pointers, 16-byte aligned) from the instance table of P and the
// vertex / index arrays it points to (rules A1-A9).  Reads neither P.traversalStack nor the LDS scene cache.
hipError_t launch_hit_surface(const FrameParams &P, const void *rays, const void *hits, void *surfaces, uint64_t count, hipStream_t s);

// ---- material.hip --------------------------------------------------------------------------------------------------
// RT64_ShadeViewRayHits: `count` RT64_RAYs, their RT64_RAY_HITs and (lods != nullptr) one float lod per record -> RT64_RAY_MATERIALs (device pointers, 16-byte aligned;
// lods 4) from the instance and texture tables of P and the vertex, index and texel arrays they point to (rules H1-H12).  Reads neither P.traversalStack nor the LDS scene cache.
hipError_t launch_hit_material(const FrameParams &P, const void *rays, const void *hits, const void *lods, void *materials, uint64_t count, hipStream_t s);

// ---- raster.hip ----------------------------------------------------------------------------------------------------
size_t raster_tri_bytes(uint32_t triTotal);       // setup records of a draw list
// Triangle setup of a draw list for a w x h target, rows [y0, y1); `apply` = drawInstances' applyScissorsAndViewports (rt64_view.cpp:1225).
bool raster_setup_takes_table_inline(uint32_t instanceCount);      // short lists: the table travels in the kernel arguments (launch_raster_setup_inline), no copy
hipError_t launch_raster_setup_inline(const GpuRasterInstance *hostTable, GpuRasterInstance *deviceTable, uint32_t instanceCount, uint32_t triTotal, void *tris, int w, int h, int y0, int y1, bool apply, hipStream_t s);
hipError_t launch_raster_setup(const GpuRasterInstance *instances, uint32_t instanceCount, uint32_t triTotal, void *tris, int w, int h, int y0, int y1, bool apply, hipStream_t s);
// Shade + blend the list, in order, into the RGBA8 target; `bounds` = pixel rectangle [x0, y0, x1, y1) the list can touch.
hipError_t launch_raster_draw(const GpuRasterInstance *instances, const void *tris, uint32_t triTotal, const GpuTexture *textures, uint8_t *target,
                              int w, int y0, int y1, const int bounds[4], int stripRank, int stripCount, bool clear, hipStream_t s);       // clear: the whole target starts as 0 (no memset in front)
// One launch for what a frame with changed tables queues before its first pass: the frame-table upload (read from the pinned upload ring) + the setup of short draw lists.
#define RASTER_PROLOGUE_LISTS 3
#define RASTER_PROLOGUE_INSTANCES 8
#define RASTER_PROLOGUE_COPY_WORDS (4096u)          // 64 KB of frame tables: beyond that the copy engine's launch is the smaller part
struct RasterPrologueList { GpuRasterInstance inst[RASTER_PROLOGUE_INSTANCES]; GpuRasterInstance *deviceTable; void *tris; uint32_t instanceCount, triTotal; int32_t w, h, y0, y1, apply; uint32_t firstBlock; };
struct RasterPrologue { RasterPrologueList list[RASTER_PROLOGUE_LISTS]; const void *copySrc; void *copyDst; uint32_t copyWords, copyBlocks, listCount, pad; };
static_assert(sizeof(RasterPrologue) <= 3584, "frame_prologue_kernel's arguments");
bool frame_prologue_takes(const RasterPrologue &a);
hipError_t launch_frame_prologue(RasterPrologue &a, hipStream_t s);

// ---- svgf.hip ------------------------------------------------------------------------------------------------------
// variance estimate + 5 a-trous iterations over the GI buffer; result in filteredIndirect[1]
#define SVGF_HALO_ROWS 66            // rows of neighbourhood the SVGF result of a row depends on (62 a-trous + 3 variance + 1 gradient)
#define GAUSSIAN_HALO_ROWS 5         // five 3x3 passes
#define SVGF_ATROUS_HALO_ROWS 62     // rows of a-trous INPUT (variance image + guide records) the result of a row depends on: what a halo exchange ships
#define SVGF_INPUT_HALO_ROWS 4       // rows of G-buffer + GI around the rows whose a-trous input is made (3 variance taps + 1 depth gradient)
hipError_t launch_svgf_inputs(const ViewImages &I, int cur, int width, int height, int gy0, int gy1, int vy0, int vy1, bool inputByResolve, hipStream_t s);      // inputByResolve: bounce_resolve_kernel wrote the filter input and marked the young pixels (ViewImages::svgfYoung)
// Compose folded into the last a-trous iteration (svgf.hip): what compose_post_kernel<false> reads and writes, for the rows [oy0, oy1) of the frame
struct SvgfComposeFold { const uint8_t *diffuse; const uint16_t *filteredDirect, *reflection, *refraction, *transparent; float *output; uint8_t *final; int oy0, oy1, writeFinal;
                         float *sppSum; int sppSub, sppCount; };      // extension primary_spp (rule P3): the composed value goes into the running sum of the frame's sub-frames; the last one stores the mean and the back buffer (sppCount <= 1: off)
hipError_t launch_svgf_atrous(const ViewImages &I, int width, int height, int y0, int y1, int oy0, int oy1, int first, int last, const SvgfComposeFold *fold, hipStream_t s);

// ---- upscale.hip ---------------------------------------------------------------------------------------------------
// Temporal upscaler stage (Upscaler::upscale, rt64_view.cpp:1584-1618): rtOutput + flow + masks + depth (render size rw x rh, jitter jx / jy)
// and the previous upscaled image -> `out` (display size dw x dh, RGBA32F: colour + accumulated frame count).
hipError_t launch_taa_upsample(const ViewImages &I, int cur, int rw, int rh, float jx, float jy, const float *prev, float *out, int dw, int dh, bool haveHistory, hipStream_t s);
// RCAS sharpening of the upscaled image (RT64_VIEW_DESC.upscalerSharpness; rules S1-S7): `in` -> `out`, both display size RGBA32F, in != out;
// k = 2^(2 min(sharpness, 1) - 2) of rule S1.  Alpha (the frame count) is copied.
hipError_t launch_rcas_sharpen(const float *in, float *out, int dw, int dh, float k, hipStream_t s);

// ---- gather.hip -----------------------------------------------------------------------------------------------------
// Rank 0 of a multi-GPU gather: frame row y <- row gather_row_owner(y) of the owner's packed buffer (`own` for rank 0, bucket + r * slotBytes for rank r).
hipError_t launch_gather_assemble(const uint8_t *own, const uint8_t *bucket, size_t slotBytes, uint8_t *frame, int width, const GatherLayout &L, hipStream_t s);
hipError_t launch_row_hit_count(const int32_t *hitInstance, uint32_t *counts, int width, int height, hipStream_t s);      // counts[y] = pixels of row y whose primary ray hit geometry

// ---- alpha_query.hip -----------------------------------------------------------------------------------------------
// RT64_TraceViewRaysAlpha: `count` RT64_RAYs and (lods != nullptr) one float lod per ray -> RT64_RAY_HITs; RT64_TraceViewRayVisibility: RT64_RAYs -> RT64_RAY_VISIBILITYs
// (device pointers, 16-byte aligned; lods 4) against the tables of P (rules K1-K10).  P.traversalStack as for launch_ray_query; both read the texture table of P as well.
hipError_t launch_alpha_query(const FrameParams &P, const void *rays, const void *lods, void *hits, uint64_t count, uint32_t flags, hipStream_t s);
hipError_t launch_visibility_query(const FrameParams &P, const void *rays, void *visibility, uint64_t count, uint32_t flags, hipStream_t s);

// ---- lighting.hip ---------------------------------------------------------------------------------------------------
// RT64_LightViewRayHits: `count` RT64_RAYs, their RT64_RAY_HITs and (lods != nullptr) one float lod per record -> RT64_RAY_LIGHTINGs (device pointers, 16-byte aligned;
// lods 4) from the instance, texture and light tables of P, with one shadow walk per admitted light (rules P1-P11).  P.traversalStack as for launch_ray_query.
hipError_t launch_hit_light(const FrameParams &P, const void *rays, const void *hits, const void *lods, void *lighting, uint64_t count, hipStream_t s);

// ---- sampled_lighting.hip -------------------------------------------------------------------------------------------
// RT64_SampleViewRayLights: `count` RT64_RAYs, their RT64_RAY_HITs, (lods != nullptr) one float lod and (keys != nullptr) one RT64_LIGHT_SAMPLE_KEY per record ->
// RT64_RAY_SAMPLED_LIGHTINGs (device pointers, 16-byte aligned; lods 4): the frame's light loop with `maxLights` draws and `diSamples` disc samples, one shadow walk per
// sample (rules J1-J11).  keys == nullptr: record i is keyed as pixel first + i of the frame, row by row.  P.traversalStack as for launch_ray_query.
hipError_t launch_hit_sampled_light(const FrameParams &P, const void *rays, const void *hits, const void *lods, const void *keys, uint64_t first, uint32_t maxLights, uint32_t diSamples,
                                    void *records, uint64_t count, hipStream_t s);

// ---- footprint.hip --------------------------------------------------------------------------------------------------
// RT64_GenerateViewCameraRays: `count` pixels (x, y pairs of uint32, 8-byte aligned; nullptr: record i is pixel n = firstPixel + i of the frame, (n % P.width, n / P.width), and firstPixel + count <= P.width * P.height) -> the
// RT64_RAYs the frame of P traced for them and (diffs != nullptr) their RT64_RAY_DIFFERENTIALs (device pointers, 16-byte aligned; rules F1-F3).  Reads only P.
hipError_t launch_camera_rays(const FrameParams &P, const void *pixels, uint64_t firstPixel, void *rays, void *diffs, uint64_t count, hipStream_t s);
// RT64_FootprintViewRayHits: `count` RT64_RAYs, their RT64_RAY_DIFFERENTIALs (nullptr: all 0) and RT64_RAY_HITs -> RT64_RAY_FOOTPRINTs (device pointers, 16-byte aligned) from the
// instance and texture tables of P and the vertex and index arrays they point to; no texel is read (rules F4-F8).  Reads neither P.traversalStack nor the LDS scene cache.
hipError_t launch_hit_footprint(const FrameParams &P, const void *rays, const void *diffs, const void *hits, void *footprints, uint64_t count, hipStream_t s);

// ---- bounce.hip -----------------------------------------------------------------------------------------------------
// RT64_BounceViewRayHits: `count` RT64_RAYs, their RT64_RAY_HITs and (lods != nullptr) one float lod per record -> RT64_RAY_BOUNCEs, reflected RT64_RAYs and refracted RT64_RAYs
// (device pointers, 16-byte aligned; lods 4; an output that is nullptr is not written) from the instance and texture tables of P (rules R1-R6).  carryCounters: the records
// take the hits' traversal counters (the hits come from the walk of the same call), otherwise 0 (R8).  Reads neither P.traversalStack nor the LDS scene cache.
hipError_t launch_hit_bounce(const FrameParams &P, const void *rays, const void *hits, const void *lods, void *bounces, void *reflected, void *refracted, uint64_t count, bool carryCounters, hipStream_t s);
// RT64_TraceViewRayMirrorChains: `count` RT64_RAYs and (lods != nullptr) their lods -> depth * count RT64_RAY_HITs and RT64_RAY_BOUNCEs, segment-major (rule R7); 1 <= depth <= 8.
// P.traversalStack as for launch_ray_query; reads the texture table of P as well.
hipError_t launch_mirror_chain(const FrameParams &P, const void *rays, const void *lods, void *hits, void *bounces, uint64_t count, uint32_t depth, uint32_t flags, hipStream_t s);

// ---- layers.hip -----------------------------------------------------------------------------------------------------
// RT64_TraceViewRayLayers: `count` RT64_RAYs and (lods != nullptr) their lods -> maxLayers * count RT64_RAY_HITs, layer-major, and `count` RT64_RAY_LAYERS (device pointers,
// 16-byte aligned; lods 4; rules T1-T6); 1 <= maxLayers <= 16.  slab: ray_layer_slab_bytes() of device memory, 16-byte aligned, that no other launch uses meanwhile (the
// payloads of the lists while they are built; nothing in it outlives the launch).  P.traversalStack as for launch_ray_query; reads the texture table of P as well.
size_t ray_layer_slab_bytes();
hipError_t launch_layer_walk(const FrameParams &P, const void *rays, const void *lods, void *hits, void *layers, void *slab, uint64_t count, uint32_t maxLayers, uint32_t flags, hipStream_t s);
// RT64_WeighViewRayLayers: `count` RT64_RAYs, their maxLayers * count RT64_RAY_HITs and (lods != nullptr) their lods -> maxLayers * count floats and `count` RT64_RAY_COVERAGEs
// (device pointers, 16-byte aligned; lods and weights 4; rule T7).  Reads neither P.traversalStack nor the LDS scene cache.
hipError_t launch_layer_weight(const FrameParams &P, const void *rays, const void *hits, const void *lods, void *weights, void *coverage, uint64_t count, uint32_t maxLayers, hipStream_t s);

// ---- radiance.hip ---------------------------------------------------------------------------------------------------
// RT64_SkyViewRays: `count` RT64_RAYs -> RT64_RAY_SKYs (device pointers, 16-byte aligned; rule W1).  Reads P, the sky texture of P's texture table, its tiled copy and
// the frame's background image; no mesh, no stack.
hipError_t launch_ray_sky(const FrameParams &P, const void *rays, void *sky, uint64_t count, hipStream_t s);
// RT64_SkyViewPixels: `count` pixels as launch_camera_rays takes them (nullptr: record i is pixel firstPixel + i of the frame) -> RT64_RAY_SKYs (rule W2).
hipError_t launch_pixel_sky(const FrameParams &P, const void *pixels, uint64_t firstPixel, void *sky, uint64_t count, hipStream_t s);
// RT64_ComposeViewRayRadiance: `count` RT64_RAYs, their maxLayers * count RT64_RAY_HITs, layer-major, and (lods != nullptr) their lods -> RT64_RAY_RADIANCEs (device pointers,
// 16-byte aligned; lods 4; rules W3-W7); 1 <= maxLayers <= 16.  flags: RT64_RADIANCE_FLAG_*.  One shadow walk per admitted light of the lit layer unless UNSHADOWED:
// P.traversalStack as for launch_ray_query.
hipError_t launch_ray_radiance(const FrameParams &P, const void *rays, const void *hits, const void *lods, void *radiance, uint64_t count, uint32_t maxLayers, uint32_t flags, hipStream_t s);

// ---- indirect.hip ---------------------------------------------------------------------------------------------------
// The links of the GI chain (include/rt64_indirect.h; rules Y1-Y12); device pointers, 16-byte aligned.  Ray i of a launch belongs to point i % points (key keys[i % points],
// or -- keys == nullptr -- pixel first + i % points of the frame, row by row) and is sample slot slotTop - i / points of it; points < count only with count < 2^32.
// RT64_GenerateViewPointGIRays: `count` bounce rays (Y4).  source: 16-byte words, the position word of source record r at source[r * strideWords], its normal word behind it;
// perRay: record i belongs to ray i, otherwise to the ray's point; a record is used if its flags hold needFlags and none of refuseFlags.  giSamples >= 1.  Reads only P.
hipError_t launch_gi_rays(const FrameParams &P, const void *source, uint32_t strideWords, bool perRay, uint32_t needFlags, uint32_t refuseFlags, const void *keys, uint64_t first,
                          uint64_t points, uint32_t giSamples, uint32_t slotTop, bool second, void *rays, uint64_t count, hipStream_t s);
// RT64_ComposeViewGIRays: `count` RT64_RAYs and their maxLayers * count RT64_RAY_HITs, layer-major -> RT64_GI_SAMPLEs (Y5-Y7); incoming: 3 floats per ray at
// incoming[i * incomingStride] (4-byte aligned), or nullptr.  light = false: the resolve alone (position, normal, instance, flags; radiance 0), no walk.  Otherwise one shadow
// walk per disc sample: P.traversalStack as for launch_ray_query.
hipError_t launch_gi_shade(const FrameParams &P, const void *rays, const void *hits, uint32_t maxLayers, const void *keys, uint64_t first, uint64_t points, const void *incoming,
                           uint32_t incomingStride, uint32_t diSamples, bool light, void *samples, uint64_t count, hipStream_t s);
// Y10: `count` RT64_RAYs, their RT64_RAY_HITs and (lods != nullptr) their lods -> RT64_GI_POINTs.  Reads neither P.traversalStack nor the LDS scene cache.
hipError_t launch_gi_points(const FrameParams &P, const void *rays, const void *hits, const void *lods, void *points, uint64_t count, hipStream_t s);
// Y8: `count` RT64_GI_POINTs and giSamples * count RT64_GI_SAMPLEs, sample-major (secondSamples: the second bounces', or nullptr; firstWalks / secondWalks: the
// RT64_RAY_LAYERS of the rays' walks, for their counters, or nullptr) -> RT64_POINT_INDIRECTs.
hipError_t launch_gi_accumulate(const FrameParams &P, const void *points, const void *firstSamples, const void *secondSamples, const void *firstWalks, const void *secondWalks,
                                uint32_t giSamples, void *records, uint64_t count, hipStream_t s);
