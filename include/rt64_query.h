/*
 * rt64_query.h -- batched ray queries against the scene a view last drew (MI355X extension of librt64.so).
 *
 * A host that has drawn a frame can cast rays of its own through the same acceleration structures and the same
 * traversal the frame's rays used: line-of-sight and camera-collision probes, picking at arbitrary points, depth
 * or lidar-style sensors.  The functions live in this header of their own (not in rt64.h's RT64_EXT_API_LIST) and
 * are resolved with their own loader, RT64_LoadLibraryQuery, from the handle RT64_LoadLibrary returned.
 *
 * Semantics (rules Q1-Q7):
 *   Q1 every ray goes through the TLAS and into each instance's object space exactly as a frame's rays do; direction need
 *      not be normalised, t is in units of |direction|, a hit needs tMin < t < tMax.
 *   Q2 default: closest hit; every intersection commits (DXR FORCE_OPAQUE: no alpha, texture-edge or depth-bias rule).
 *   Q3 RT64_RAY_FLAG_ACCEPT_FIRST_HIT: the walk ends at the first intersection it finds (an occlusion query).
 *   Q4 RT64_RAY_FLAG_CULL_BACK_FACING: back-facing triangles are skipped, except on instances with
 *      RT64_INSTANCE_DISABLE_BACKFACE_CULLING.
 *   Q5 a miss is instance = -1, primitive = 0xFFFFFFFF, t = +inf, u = v = 0.  instance = TLAS build position (the index
 *      RT64_IMAGE_PRIMARY_HIT carries; RT64_GetViewRaytracedInstance turns it into a handle), primitive = triangle number
 *      in the mesh as the host sent it.  nodesVisited / trianglesTested: device option count_traversal = 1, else 0.
 *   Q6 a ray with a NaN anywhere, an inf in origin or direction, tMin >= tMax or a zero direction misses.
 *   Q7 queries see the tables and BLASes of the view's last RT64_DrawDevice.  They are refused (0, RT64_GetLastError set)
 *      before the view's first frame, and after RT64_SetMesh / RT64_DestroyMesh on a mesh that frame traced, until the
 *      next draw.  The device's tile / interleave partition does not apply: the whole scene is queried.
 */
#ifndef RT64_QUERY_H_INCLUDED
#define RT64_QUERY_H_INCLUDED

#include "rt64.h"

typedef struct { float origin[3]; float tMin; float direction[3]; float tMax; } RT64_RAY;                 /* 32 B */
typedef struct { float t, u, v; int instance; unsigned int primitive;
                 unsigned int nodesVisited, trianglesTested, reserved; } RT64_RAY_HIT;                     /* 32 B */

#define RT64_RAY_FLAG_CULL_BACK_FACING   0x1
#define RT64_RAY_FLAG_ACCEPT_FIRST_HIT   0x2

#define RT64_QUERY_API_LIST(X) \
    /* `count` rays in host memory -> `count` hits in host memory.  Returns 1 after the hits are written, or 0 with RT64_GetLastError set. */ \
    X(TraceViewRays, RT64_TraceViewRays, int, (RT64_VIEW *view, const RT64_RAY *rays, RT64_RAY_HIT *hits, size_t count, unsigned int flags)) \
    /* The same on device memory (16-byte aligned; e.g. torch tensors).  stream = NULL: on the device's stream, and the call returns after \
       completion.  Otherwise the call enqueues the query on `stream` (a hipStream_t) behind the view's last frame and returns at once; \
       the frame's tables and BLASes are kept until the query has run. */ \
    X(TraceViewRaysDevice, RT64_TraceViewRaysDevice, int, (RT64_VIEW *view, const void *rays, void *hits, size_t count, unsigned int flags, void *stream)) \
    /* Instance index of a hit (or of RT64_IMAGE_PRIMARY_HIT) -> the instance handle of the view's last frame; NULL when out of range. */ \
    X(GetViewRaytracedInstance, RT64_GetViewRaytracedInstance, RT64_INSTANCE *, (RT64_VIEW *view, int instance))

#define RT64_X(member, symbol, ret, args) typedef ret (*member##Ptr) args;
RT64_QUERY_API_LIST(RT64_X)
#undef RT64_X

typedef struct {
#define RT64_X(member, symbol, ret, args) member##Ptr member;
    RT64_QUERY_API_LIST(RT64_X)
#undef RT64_X
} RT64_LIBRARY_QUERY;

RT64_INLINE RT64_LIBRARY_QUERY RT64_LoadLibraryQuery(RT64_LIBRARY lib) {
    RT64_LIBRARY_QUERY q;
#define RT64_X(member, symbol, ret, args) q.member = lib.handle ? (member##Ptr)(RT64_DLSYM(lib.handle, #symbol)) : 0;
    RT64_QUERY_API_LIST(RT64_X)
#undef RT64_X
    return q;
}

RT64_STATIC_ASSERT(sizeof(RT64_RAY) == 32, "RT64_RAY");
RT64_STATIC_ASSERT(offsetof(RT64_RAY, tMin) == 12, "RT64_RAY.tMin");
RT64_STATIC_ASSERT(offsetof(RT64_RAY, direction) == 16, "RT64_RAY.direction");
RT64_STATIC_ASSERT(offsetof(RT64_RAY, tMax) == 28, "RT64_RAY.tMax");
RT64_STATIC_ASSERT(sizeof(RT64_RAY_HIT) == 32, "RT64_RAY_HIT");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_HIT, instance) == 12, "RT64_RAY_HIT.instance");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_HIT, primitive) == 16, "RT64_RAY_HIT.primitive");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_HIT, nodesVisited) == 20, "RT64_RAY_HIT.nodesVisited");
RT64_STATIC_ASSERT(offsetof(RT64_RAY_HIT, trianglesTested) == 24, "RT64_RAY_HIT.trianglesTested");

#endif /* RT64_QUERY_H_INCLUDED */
