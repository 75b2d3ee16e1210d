// mipgen.hip -- mip chains of RGBA8 textures (device option generate_mipmaps).
//
// The reference sizes an RGBA8 texture for a full chain (rt64_texture.cpp:38) and meant to fill it with GenerateMipsCS.hlsl, but disables
// that on AMD adapters and compiles it out everywhere else (rt64_device.cpp:181-186, 758-762).  The shader is no usable definition (its
// border weights divide 0 by 0 when the 1x1 level is made in the same pass as a larger one, BorderUV point-samples the edge ring, and odd
// sizes lean on the hardware bilinear filter's precision), so the library fixes its own integer rule:
//   M1 Scope      option generate_mipmaps (0 / 1, default 0) applies to RGBA8 textures created by RT64_CreateTexture while it is 1; textures made
//                 earlier and DDS textures keep their levels; blue noise, gBackground and the sky lookup are untouched.
//   M2 Levels     L = min(floor(log2(max(w, h))) + 1, RT64_MAX_MIPS); level m is max(1, w >> m) x max(1, h >> m), packed back to back through
//                 mipOffset exactly like the levels of a DDS file.
//   M3 Footprint  level m >= 1 is made from the STORED 8-bit level m - 1.  Per axis, source size s, destination index x:
//                   s = 1: tap {0}, weight (1), D = 1
//                   s even: taps {2x, 2x + 1}, weights (1, 1), D = 2
//                   s odd >= 3, n = (s - 1) / 2: taps {2x, 2x + 1, 2x + 2}, weights (n - x, n, x + 1), D = s
//                 the exact area average of the destination texel's footprint; every tap lies inside the level (no addressing mode).
//   M4 Arithmetic per channel, t = (sum_i sum_j wx_i wy_j src_ij + (Dx Dy) / 2) / (Dx Dy) in unsigned integers (64-bit where 255 Dx Dy can
//                 pass 2^32); ties round up.  Even x even sources: (a + b + c + d + 2) >> 2.
//   M5 Alpha      minAlpha / maxAlpha (opacity rules O1 / O2) stay those of level 0: M4 rounds a convex combination to nearest, so no level
//                 leaves level 0's alpha bounds.
//   M6 Sampling   unchanged: T3 (shade.h, tex_sample_grad) picks the level; power-of-two textures stay power of two at every level.
//
// Launch shapes.  Texture creation waits on the stream (rt64_texture.cpp:130-137), so the launch count is the cost of a small texture:
//   - a chain whose next level holds at most MIPGEN_TAIL_TEXELS texels (every texture up to 128 x 128) is ONE launch of ONE workgroup
//     (mipgen_tail_kernel): the first level is read from HBM, every level it makes goes to LDS and HBM, one barrier per level;
//   - larger levels take one grid launch each (mipgen_level_kernel, MIPGEN_GRID_TEXELS destination texels per thread; the source level was
//     just written and is still in L2 / MALL) until the next level fits the one-workgroup tail, which makes the rest.
#include "kernels.h"

namespace {

struct MipLevel { uint32_t offset, w, h; };      // offset in texels (Texture::mipOffset)
struct MipChain { MipLevel level[RT64_MAX_MIPS]; uint32_t first, last; };      // the tail reads level `first` from HBM and makes first + 1 .. last

#define MIPGEN_TAIL_THREADS 1024u
#define MIPGEN_GRID_THREADS 256u
#define MIPGEN_GRID_TEXELS 4u

// M4 for an even x even source: four taps of weight 1, D = 4, both byte pairs of a texel at once (16-bit lanes: 4 * 255 + 2 fits)
__device__ inline uint32_t avg4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
    const uint32_t m = 0x00FF00FFu;
    const uint32_t lo = (a & m) + (b & m) + (c & m) + (d & m) + 0x00020002u;
    const uint32_t hi = ((a >> 8) & m) + ((b >> 8) & m) + ((c >> 8) & m) + ((d >> 8) & m) + 0x00020002u;
    return ((lo >> 2) & m) | (((hi >> 2) & m) << 8);
}

// M3 along one axis: first tap, tap count, weights, divisor
struct Taps { uint32_t t0, n, w[3], D; };
__device__ inline Taps axis_taps(uint32_t s, uint32_t x) {
    if (s == 1) return { 0u, 1u, { 1u, 0u, 0u }, 1u };
    if (!(s & 1u)) return { 2u * x, 2u, { 1u, 1u, 0u }, 2u };
    const uint32_t n = (s - 1u) >> 1;
    return { 2u * x, 3u, { n - x, n, x + 1u }, s };
}

// M3 + M4 for any source size; Acc = uint32_t while 255 Dx Dy + (Dx Dy) / 2 fits, else uint64_t
template <class Acc>
__device__ inline uint32_t box_texel(const uint32_t *src, uint32_t sw, uint32_t sh, uint32_t x, uint32_t y) {
    const Taps tx = axis_taps(sw, x), ty = axis_taps(sh, y);
    Acc c[4] = { 0, 0, 0, 0 };
#pragma unroll
    for (uint32_t j = 0; j < 3; j++) {
        if (j >= ty.n) break;
        const uint32_t *row = src + (size_t)(ty.t0 + j) * sw + tx.t0;
#pragma unroll
        for (uint32_t i = 0; i < 3; i++) {
            if (i >= tx.n) break;
            const uint32_t p = row[i];
            const Acc w = (Acc)tx.w[i] * (Acc)ty.w[j];
#pragma unroll
            for (int k = 0; k < 4; k++) c[k] += w * (Acc)((p >> (8 * k)) & 255u);
        }
    }
    const Acc D = (Acc)tx.D * (Acc)ty.D, half = D / 2;
    uint32_t out = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) out |= (uint32_t)((c[k] + half) / D) << (8 * k);
    return out;
}

enum { MIP_EVEN = 0, MIP_ODD32 = 1, MIP_ODD64 = 2 };
__device__ inline int level_kind(uint32_t sw, uint32_t sh) {
    if (!(sw & 1u) && !(sh & 1u)) return MIP_EVEN;
    const uint64_t D = (uint64_t)(sw == 1 ? 1u : (sw & 1u) ? sw : 2u) * (uint64_t)(sh == 1 ? 1u : (sh & 1u) ? sh : 2u);
    return 255u * D + D / 2 <= 0xFFFFFFFFull ? MIP_ODD32 : MIP_ODD64;
}

__device__ inline uint32_t mip_texel(const uint32_t *src, uint32_t sw, uint32_t sh, int kind, uint32_t x, uint32_t y) {
    if (kind == MIP_EVEN) {
        const uint32_t *r0 = src + (size_t)(2u * y) * sw + 2u * x, *r1 = r0 + sw;
        return avg4(r0[0], r0[1], r1[0], r1[1]);
    }
    return kind == MIP_ODD32 ? box_texel<uint32_t>(src, sw, sh, x, y) : box_texel<uint64_t>(src, sw, sh, x, y);
}

// One level of a large texture: s -> d, MIPGEN_GRID_TEXELS destination texels per thread (strided by the workgroup: coalesced stores).
__global__ __launch_bounds__(MIPGEN_GRID_THREADS) void mipgen_level_kernel(uint32_t *__restrict__ texels, MipLevel s, MipLevel d) {
    const uint32_t n = d.w * d.h, base = blockIdx.x * (MIPGEN_GRID_THREADS * MIPGEN_GRID_TEXELS) + threadIdx.x;
    const uint32_t *src = texels + s.offset;
    uint32_t *dst = texels + d.offset;
    const int kind = level_kind(s.w, s.h);
    // even x even with an even level offset: the two taps of a row are one 8-byte load (rows start even: s.w is even)
    const bool pairs = kind == MIP_EVEN && !(s.offset & 1u);
#pragma unroll
    for (uint32_t k = 0; k < MIPGEN_GRID_TEXELS; k++) {
        const uint32_t i = base + k * MIPGEN_GRID_THREADS;
        if (i >= n) break;
        const uint32_t y = i / d.w, x = i - y * d.w;
        if (pairs) {
            const uint2 a = *reinterpret_cast<const uint2 *>(src + (size_t)(2u * y) * s.w + 2u * x);
            const uint2 b = *reinterpret_cast<const uint2 *>(src + (size_t)(2u * y + 1u) * s.w + 2u * x);
            dst[i] = avg4(a.x, a.y, b.x, b.y);
        }
        else dst[i] = mip_texel(src, s.w, s.h, kind, x, y);
    }
}

// The rest of a chain in one workgroup: level c.first from HBM, then every level from the one before it in LDS.  buf0 holds the levels
// first + 1, first + 3, ... (at most MIPGEN_TAIL_TEXELS texels), buf1 the others (a level has at most half the texels of the one before).
__global__ __launch_bounds__(MIPGEN_TAIL_THREADS) void mipgen_tail_kernel(uint32_t *__restrict__ texels, MipChain c) {
    __shared__ uint32_t buf0[MIPGEN_TAIL_TEXELS], buf1[MIPGEN_TAIL_TEXELS / 2];
    {
        const MipLevel s = c.level[c.first], d = c.level[c.first + 1];
        const uint32_t *src = texels + s.offset;
        uint32_t *dst = texels + d.offset;
        const int kind = level_kind(s.w, s.h);
        for (uint32_t i = threadIdx.x; i < d.w * d.h; i += MIPGEN_TAIL_THREADS) {
            const uint32_t y = i / d.w, x = i - y * d.w;
            const uint32_t v = mip_texel(src, s.w, s.h, kind, x, y);
            buf0[i] = v; dst[i] = v;
        }
    }
    for (uint32_t m = c.first + 2; m <= c.last; m++) {
        __syncthreads();
        const bool odd = ((m - c.first) & 1u) != 0;
        const uint32_t *src = odd ? buf1 : buf0;
        uint32_t *out = odd ? buf0 : buf1;
        const MipLevel s = c.level[m - 1], d = c.level[m];
        uint32_t *dst = texels + d.offset;
        const int kind = level_kind(s.w, s.h);
        for (uint32_t i = threadIdx.x; i < d.w * d.h; i += MIPGEN_TAIL_THREADS) {
            const uint32_t y = i / d.w, x = i - y * d.w;
            const uint32_t v = mip_texel(src, s.w, s.h, kind, x, y);
            out[i] = v; dst[i] = v;
        }
    }
}

}  // namespace

int mipgen_level_count(int width, int height) {
    int L = 1;
    for (int s = std::max(width, height); s > 1; s >>= 1) L++;
    return std::min(L, RT64_MAX_MIPS);
}

hipError_t mipgen_launch(uint8_t *texels, const uint32_t *mipOffset, uint32_t width, uint32_t height, int levels, hipStream_t stream) {
    if (levels < 1 || levels > RT64_MAX_MIPS || width == 0 || height == 0) return hipErrorInvalidValue;
    MipChain c = {};
    for (int m = 0; m < levels; m++) c.level[m] = { mipOffset[m], std::max(width >> m, 1u), std::max(height >> m, 1u) };
    uint32_t *t = reinterpret_cast<uint32_t *>(texels);
    int m = 0;
    for (; m + 1 < levels && c.level[m + 1].w * c.level[m + 1].h > MIPGEN_TAIL_TEXELS; m++) {
        const uint32_t n = c.level[m + 1].w * c.level[m + 1].h, per = MIPGEN_GRID_THREADS * MIPGEN_GRID_TEXELS;
        hipLaunchKernelGGL(mipgen_level_kernel, dim3((n + per - 1) / per), dim3(MIPGEN_GRID_THREADS), 0, stream, t, c.level[m], c.level[m + 1]);
    }
    if (m + 1 < levels) {
        c.first = (uint32_t)m; c.last = (uint32_t)(levels - 1);
        hipLaunchKernelGGL(mipgen_tail_kernel, dim3(1), dim3(MIPGEN_TAIL_THREADS), 0, stream, t, c);
    }
    return hipGetLastError();
}
