"""ctypes mirror of include/rt64.h -- the RT64 C-ABI function-pointer table, bound the way a host binds it.

The product is librt64.so (HIP); this module is only the Python-side harness used by tests/, bench.py and
__graft_entry__.py to drive it through the same 33 exported symbols a C host resolves with dlsym
(/root/reference/src/rt64lib/public/rt64.h:305-402), plus the additive RT64_* extensions.
It contains no rendering code and never falls back to a CPU path: if librt64.so is missing, loading raises.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIBRARY = os.path.join(_HERE, "librt64.so")

# ---- constants (include/rt64.h) -----------------------------------------------------------------------------
MESH_RAYTRACE_ENABLED, MESH_RAYTRACE_UPDATABLE, MESH_RAYTRACE_FAST_TRACE, MESH_RAYTRACE_COMPACT = 0x1, 0x2, 0x4, 0x8
SHADER_FILTER_POINT, SHADER_FILTER_LINEAR = 0, 1
SHADER_ADDRESSING_WRAP, SHADER_ADDRESSING_MIRROR, SHADER_ADDRESSING_CLAMP = 0, 1, 2
SHADER_RASTER_ENABLED, SHADER_RAYTRACE_ENABLED, SHADER_NORMAL_MAP_ENABLED, SHADER_SPECULAR_MAP_ENABLED = 0x1, 0x2, 0x4, 0x8
INSTANCE_RASTER_BACKGROUND, INSTANCE_DISABLE_BACKFACE_CULLING = 0x1, 0x2
LIGHT_GROUP_MASK_ALL, LIGHT_GROUP_DEFAULT = 0xFFFFFFFF, 0x1
TEXTURE_FORMAT_RGBA8, TEXTURE_FORMAT_DDS = 0x1, 0x2
UPSCALER_OFF, UPSCALER_AUTO, UPSCALER_DLSS, UPSCALER_FSR, UPSCALER_XESS = range(5)
(UPSCALER_MODE_AUTO, UPSCALER_MODE_ULTRA_PERFORMANCE, UPSCALER_MODE_PERFORMANCE, UPSCALER_MODE_BALANCED, UPSCALER_MODE_QUALITY,
 UPSCALER_MODE_ULTRA_QUALITY, UPSCALER_MODE_NATIVE) = range(7)
ACCEL_NODES, ACCEL_TRIANGLES, ACCEL_SORTED_INDEX, ACCEL_MORTON, ACCEL_HEADER, ACCEL_HOST_DEPTH = range(6)

(IMAGE_FINAL_RGBA8, IMAGE_SHADING_POSITION, IMAGE_SHADING_NORMAL, IMAGE_SHADING_SPECULAR, IMAGE_DIFFUSE,
 IMAGE_INSTANCE_ID, IMAGE_DIRECT_LIGHT_RAW, IMAGE_DIRECT_LIGHT_FILTERED, IMAGE_INDIRECT_LIGHT_RAW,
 IMAGE_INDIRECT_LIGHT_FILTERED, IMAGE_REFLECTION, IMAGE_REFRACTION, IMAGE_TRANSPARENT, IMAGE_FLOW,
 IMAGE_REACTIVE_MASK, IMAGE_LOCK_MASK, IMAGE_DEPTH, IMAGE_OUTPUT_RGBA32F, IMAGE_PRIMARY_HIT,
 IMAGE_VIEW_DIRECTION, IMAGE_FIRST_INSTANCE_ID, IMAGE_BACKGROUND, IMAGE_UPSCALED,
 IMAGE_GI_MOMENTS, IMAGE_FILTER_GUIDE, IMAGE_FILTER_PING, IMAGE_SHARPENED) = range(27)

# image id -> (numpy dtype string, channels)
IMAGE_FORMATS = {
    IMAGE_FINAL_RGBA8: ("u1", 4), IMAGE_SHADING_POSITION: ("f4", 4), IMAGE_SHADING_NORMAL: ("f4", 4),
    IMAGE_SHADING_SPECULAR: ("f4", 4), IMAGE_DIFFUSE: ("f4", 4), IMAGE_INSTANCE_ID: ("i4", 1),
    IMAGE_DIRECT_LIGHT_RAW: ("f4", 4), IMAGE_DIRECT_LIGHT_FILTERED: ("f4", 4), IMAGE_INDIRECT_LIGHT_RAW: ("f4", 4),
    IMAGE_INDIRECT_LIGHT_FILTERED: ("f4", 4), IMAGE_REFLECTION: ("f4", 4), IMAGE_REFRACTION: ("f4", 4),
    IMAGE_TRANSPARENT: ("f4", 4), IMAGE_FLOW: ("f4", 2), IMAGE_REACTIVE_MASK: ("f4", 1), IMAGE_LOCK_MASK: ("f4", 1),
    IMAGE_DEPTH: ("f4", 1), IMAGE_OUTPUT_RGBA32F: ("f4", 4), IMAGE_PRIMARY_HIT: ("u4", 4),
    IMAGE_VIEW_DIRECTION: ("f4", 4), IMAGE_FIRST_INSTANCE_ID: ("i4", 1), IMAGE_BACKGROUND: ("u1", 4), IMAGE_UPSCALED: ("f4", 4),
    IMAGE_GI_MOMENTS: ("f4", 2), IMAGE_FILTER_GUIDE: ("u4", 4), IMAGE_FILTER_PING: ("f4", 4),
    IMAGE_SHARPENED: ("f4", 4),
}


# ---- POD structs ------------------------------------------------------------------------------------------------
class VECTOR2(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float)]


class VECTOR3(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float)]

    def __init__(self, x=0.0, y=0.0, z=0.0):
        super().__init__(x, y, z)


class VECTOR4(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float), ("w", C.c_float)]


class MATRIX4(C.Structure):
    _fields_ = [("m", (C.c_float * 4) * 4)]

    @staticmethod
    def from_rows(rows):
        m = MATRIX4()
        for r in range(4):
            for c in range(4):
                m.m[r][c] = float(rows[r][c])
        return m

    @staticmethod
    def identity():
        return MATRIX4.from_rows([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])


class RECT(C.Structure):
    _fields_ = [("x", C.c_int), ("y", C.c_int), ("w", C.c_int), ("h", C.c_int)]


class MATERIAL(C.Structure):
    _fields_ = [("diffuseTexIndex", C.c_int), ("normalTexIndex", C.c_int), ("specularTexIndex", C.c_int),
                ("ignoreNormalFactor", C.c_float), ("uvDetailScale", C.c_float), ("reflectionFactor", C.c_float),
                ("reflectionFresnelFactor", C.c_float), ("reflectionShineFactor", C.c_float), ("refractionFactor", C.c_float),
                ("specularColor", VECTOR3), ("specularExponent", C.c_float), ("solidAlphaMultiplier", C.c_float),
                ("shadowAlphaMultiplier", C.c_float), ("depthBias", C.c_float), ("shadowRayBias", C.c_float),
                ("selfLight", VECTOR3), ("lightGroupMaskBits", C.c_uint), ("fogColor", VECTOR3),
                ("diffuseColorMix", VECTOR4), ("fogMul", C.c_float), ("fogOffset", C.c_float), ("fogEnabled", C.c_uint),
                ("lockMask", C.c_float), ("enabledAttributes", C.c_int)]


class LIGHT(C.Structure):
    _fields_ = [("position", VECTOR3), ("diffuseColor", VECTOR3), ("attenuationRadius", C.c_float), ("pointRadius", C.c_float),
                ("specularColor", VECTOR3), ("shadowOffset", C.c_float), ("attenuationExponent", C.c_float),
                ("flickerIntensity", C.c_float), ("groupBits", C.c_uint)]


class SCENE_DESC(C.Structure):
    _fields_ = [("ambientBaseColor", VECTOR3), ("ambientNoGIColor", VECTOR3), ("eyeLightDiffuseColor", VECTOR3),
                ("eyeLightSpecularColor", VECTOR3), ("skyDiffuseMultiplier", VECTOR3), ("skyHSLModifier", VECTOR3),
                ("skyYawOffset", C.c_float), ("giDiffuseStrength", C.c_float), ("giSkyStrength", C.c_float)]


class VIEW_DESC(C.Structure):
    _fields_ = [("resolutionScale", C.c_float), ("motionBlurStrength", C.c_float), ("diSamples", C.c_uint),
                ("giSamples", C.c_uint), ("maxLights", C.c_uint), ("upscaler", C.c_ubyte), ("upscalerMode", C.c_ubyte),
                ("upscalerSharpness", C.c_float), ("denoiserEnabled", C.c_bool)]


class INSTANCE_DESC(C.Structure):
    _fields_ = [("mesh", C.c_void_p), ("transform", MATRIX4), ("previousTransform", MATRIX4),
                ("diffuseTexture", C.c_void_p), ("normalTexture", C.c_void_p), ("specularTexture", C.c_void_p),
                ("shader", C.c_void_p), ("material", MATERIAL), ("scissorRect", RECT), ("viewportRect", RECT),
                ("flags", C.c_uint)]


class TEXTURE_DESC(C.Structure):
    _fields_ = [("bytes", C.c_void_p), ("byteCount", C.c_int), ("format", C.c_int), ("width", C.c_int),
                ("height", C.c_int), ("rowPitch", C.c_int)]


class FRAME_STATS(C.Structure):
    _fields_ = [("structSize", C.c_uint), ("width", C.c_uint), ("height", C.c_uint), ("tileY0", C.c_uint), ("tileY1", C.c_uint),
                ("primaryRays", C.c_ulonglong), ("shadowRays", C.c_ulonglong), ("indirectRays", C.c_ulonglong),
                ("reflectionRays", C.c_ulonglong), ("refractionRays", C.c_ulonglong),
                ("nodesVisited", C.c_ulonglong), ("trianglesTested", C.c_ulonglong),
                ("msTotal", C.c_float), ("msBuild", C.c_float), ("msPrimary", C.c_float), ("msDirect", C.c_float),
                ("msIndirect", C.c_float), ("msReflectRefract", C.c_float), ("msDenoise", C.c_float), ("msComposePost", C.c_float),
                ("msHostWall", C.c_float),
                ("blasNodeBytes", C.c_uint), ("blasTriangleBytes", C.c_uint), ("tlasNodeBytes", C.c_uint),
                ("instanceCount", C.c_uint), ("triangleCount", C.c_uint),
                ("msPrimaryTrace", C.c_float), ("msPrimaryShade", C.c_float),
                ("stripRank", C.c_uint), ("stripCount", C.c_uint), ("rowsRendered", C.c_uint), ("leanFrame", C.c_uint),
                ("nodesPrimary", C.c_ulonglong), ("trianglesPrimary", C.c_ulonglong), ("nodesDirect", C.c_ulonglong),
                ("trianglesDirect", C.c_ulonglong), ("nodesIndirect", C.c_ulonglong), ("trianglesIndirect", C.c_ulonglong),
                ("screenWidth", C.c_uint), ("screenHeight", C.c_uint), ("accumFrames", C.c_uint),
                ("accumMsTotal", C.c_float), ("accumMsBuild", C.c_float), ("accumMsPrimaryTrace", C.c_float), ("accumMsPrimaryShade", C.c_float),
                ("accumMsDirect", C.c_float), ("accumMsIndirect", C.c_float), ("accumMsReflectRefract", C.c_float), ("accumMsDenoise", C.c_float),
                ("accumMsComposePost", C.c_float), ("fusedFrame", C.c_uint), ("packedFinal", C.c_uint),
                ("overlappedFrame", C.c_uint), ("reflectionBesideDenoiser", C.c_uint), ("traversalOverflow", C.c_uint)]


assert C.sizeof(MATERIAL) == 132 and C.sizeof(LIGHT) == 60 and C.sizeof(SCENE_DESC) == 84
assert C.sizeof(VIEW_DESC) == 32 and C.sizeof(INSTANCE_DESC) == 336 and C.sizeof(TEXTURE_DESC) == 32

_P = C.c_void_p
# (member, symbol, restype, argtypes) in RT64_LIBRARY member order (include/rt64.h RT64_API_LIST)
API = [
    ("GetLastError", "RT64_GetLastError", C.c_char_p, []),
    ("CreateDevice", "RT64_CreateDevice", _P, [_P]),
    ("DestroyDevice", "RT64_DestroyDevice", None, [_P]),
    ("DrawDevice", "RT64_DrawDevice", None, [_P, C.c_int, C.c_float]),
    ("CreateView", "RT64_CreateView", _P, [_P]),
    ("SetViewPerspective", "RT64_SetViewPerspective", None, [_P, MATRIX4, C.c_float, C.c_float, C.c_float, C.c_bool]),
    ("SetViewDescription", "RT64_SetViewDescription", None, [_P, VIEW_DESC]),
    ("SetViewSkyPlane", "RT64_SetViewSkyPlane", None, [_P, _P]),
    ("GetViewRaytracedInstanceAt", "RT64_GetViewRaytracedInstanceAt", _P, [_P, C.c_int, C.c_int]),
    ("GetViewUpscalerSupport", "RT64_GetViewUpscalerSupport", C.c_bool, [_P, C.c_char]),
    ("DestroyView", "RT64_DestroyView", None, [_P]),
    ("CreateScene", "RT64_CreateScene", _P, [_P]),
    ("SetSceneDescription", "RT64_SetSceneDescription", None, [_P, SCENE_DESC]),
    ("SetSceneLights", "RT64_SetSceneLights", None, [_P, C.POINTER(LIGHT), C.c_int]),
    ("DestroyScene", "RT64_DestroyScene", None, [_P]),
    ("CreateMesh", "RT64_CreateMesh", _P, [_P, C.c_int]),
    ("SetMesh", "RT64_SetMesh", None, [_P, _P, C.c_int, C.c_int, _P, C.c_int]),
    ("DestroyMesh", "RT64_DestroyMesh", None, [_P]),
    ("CreateShader", "RT64_CreateShader", _P, [_P, C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.c_int]),
    ("DestroyShader", "RT64_DestroyShader", None, [_P]),
    ("CreateInstance", "RT64_CreateInstance", _P, [_P]),
    ("SetInstanceDescription", "RT64_SetInstanceDescription", None, [_P, INSTANCE_DESC]),
    ("DestroyInstance", "RT64_DestroyInstance", None, [_P]),
    ("CreateTexture", "RT64_CreateTexture", _P, [_P, TEXTURE_DESC]),
    ("DestroyTexture", "RT64_DestroyTexture", None, [_P]),
    ("CreateInspector", "RT64_CreateInspector", _P, [_P]),
    ("HandleMessageInspector", "RT64_HandleMessageInspector", C.c_bool, [_P, C.c_uint, C.c_size_t, C.c_ssize_t]),
    ("PrintClearInspector", "RT64_PrintClearInspector", None, [_P]),
    ("PrintMessageInspector", "RT64_PrintMessageInspector", None, [_P, C.c_char_p]),
    ("SetSceneInspector", "RT64_SetSceneInspector", None, [_P, C.POINTER(SCENE_DESC)]),
    ("SetMaterialInspector", "RT64_SetMaterialInspector", None, [_P, C.POINTER(MATERIAL), C.c_char_p]),
    ("SetLightsInspector", "RT64_SetLightsInspector", None, [_P, C.POINTER(LIGHT), C.POINTER(C.c_int), C.c_int]),
    ("DestroyInspector", "RT64_DestroyInspector", None, [_P]),
]

EXT_API = [
    ("CreateDeviceHeadless", "RT64_CreateDeviceHeadless", _P, [C.c_int, C.c_int, C.c_int]),
    ("SetDeviceSize", "RT64_SetDeviceSize", None, [_P, C.c_int, C.c_int]),
    ("SetDeviceTile", "RT64_SetDeviceTile", None, [_P, C.c_int, C.c_int]),
    ("SetDeviceInterleave", "RT64_SetDeviceInterleave", None, [_P, C.c_int, C.c_int]),
    ("ReadbackDevice", "RT64_ReadbackDevice", C.c_size_t, [_P, C.c_int, _P, C.c_size_t]),
    ("CopyDeviceImage", "RT64_CopyDeviceImage", C.c_size_t, [_P, C.c_int, _P, C.c_size_t]),
    ("GetDeviceStats", "RT64_GetDeviceStats", C.c_int, [_P, C.POINTER(FRAME_STATS)]),
    ("SetDeviceOption", "RT64_SetDeviceOption", C.c_int, [_P, C.c_char_p, C.c_double]),
    ("ReadbackTileTiming", "RT64_ReadbackTileTiming", C.c_size_t, [_P, _P, C.c_size_t]),
    ("GetDeviceStream", "RT64_GetDeviceStream", _P, [_P]),
    ("SetDeviceGatherTarget", "RT64_SetDeviceGatherTarget", None, [_P, _P, C.c_size_t]),
    ("ReadbackMeshAccel", "RT64_ReadbackMeshAccel", C.c_size_t, [_P, C.c_int, _P, C.c_size_t]),
    ("ReadbackTexture", "RT64_ReadbackTexture", C.c_size_t, [_P, C.c_int, _P, C.c_size_t]),
    ("ReadbackViewAccel", "RT64_ReadbackViewAccel", C.c_size_t, [_P, C.c_int, _P, C.c_size_t]),
    ("MeshTreeDepth", "RT64_MeshTreeDepth", C.c_uint, [_P, C.c_int, C.c_int, _P, C.c_int]),
    ("GetGatherUniqueId", "RT64_GetGatherUniqueId", C.c_int, [_P, C.c_size_t]),
    ("CreateGather", "RT64_CreateGather", _P, [_P, _P, C.c_size_t, C.c_int, C.c_int, C.c_int]),
    ("SubmitGather", "RT64_SubmitGather", C.c_int, [_P]),
    ("ReadbackGather", "RT64_ReadbackGather", C.c_size_t, [_P, C.c_int, _P, C.c_size_t, C.c_int]),
    ("GetGatherFrame", "RT64_GetGatherFrame", _P, [_P, C.c_int]),
    ("DestroyGather", "RT64_DestroyGather", None, [_P]),
    ("GetGatherDirectHandle", "RT64_GetGatherDirectHandle", C.c_size_t, [_P, _P, C.c_size_t]),
    ("SetGatherDirect", "RT64_SetGatherDirect", C.c_int, [_P, _P, C.c_size_t, C.c_int]),
    ("GatherRowOwner", "RT64_GatherRowOwner", C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    ("GatherOwnedRows", "RT64_GatherOwnedRows", C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int]),
    ("GatherSlotRows", "RT64_GatherSlotRows", C.c_int, [C.c_int, C.c_int, C.c_int]),
    ("GatherRowOwnerOf", "RT64_GatherRowOwnerOf", C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int)]),
    ("GatherOwnedRowsOf", "RT64_GatherOwnedRowsOf", C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int]),
    ("GatherSlotRowsOf", "RT64_GatherSlotRowsOf", C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_int)]),
    ("GetGatherBands", "RT64_GetGatherBands", C.c_int, [_P, C.POINTER(C.c_int), C.c_int]),
    ("BalanceGatherBands", "RT64_BalanceGatherBands", None, [C.POINTER(C.c_uint), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    ("RebalanceGatherBands", "RT64_RebalanceGatherBands", C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_int)]),
    ("SetGatherBands", "RT64_SetGatherBands", C.c_int, [_P, C.POINTER(C.c_int)]),
    ("HaloPlan", "RT64_HaloPlan", C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int, _P, C.c_int]),
    ("SetDeviceHaloExchange", "RT64_SetDeviceHaloExchange", C.c_int, [_P, _P, _P, C.POINTER(C.c_int), C.c_int, C.c_int]),
]
# include/rt64_query.h: its own list and loader (RT64_LoadLibraryQuery), not part of exported_symbols() (the rt64.h list)
QUERY_API = [
    ("TraceViewRays", "RT64_TraceViewRays", C.c_int, [_P, _P, _P, C.c_size_t, C.c_uint]),
    ("TraceViewRaysDevice", "RT64_TraceViewRaysDevice", C.c_int, [_P, _P, _P, C.c_size_t, C.c_uint, _P]),
    ("GetViewRaytracedInstance", "RT64_GetViewRaytracedInstance", _P, [_P, C.c_int]),
]
RAY_FLAG_CULL_BACK_FACING, RAY_FLAG_ACCEPT_FIRST_HIT = 0x1, 0x2
# include/rt64_surface.h: surface records for hits, again a list and a loader (RT64_LoadLibrarySurface) of its own
SURFACE_API = [
    ("ResolveViewRayHits", "RT64_ResolveViewRayHits", C.c_int, [_P, _P, _P, _P, C.c_size_t]),
    ("ResolveViewRayHitsDevice", "RT64_ResolveViewRayHitsDevice", C.c_int, [_P, _P, _P, _P, C.c_size_t, _P]),
    ("TraceViewRaySurfaces", "RT64_TraceViewRaySurfaces", C.c_int, [_P, _P, _P, _P, C.c_size_t, C.c_uint]),
]
SURFACE_VALID, SURFACE_BACK_FACE, SURFACE_HAS_UV, SURFACE_BAD_HIT = 0x1, 0x2, 0x4, 0x8
# include/rt64_material.h: material records for hits, a list and a loader (RT64_LoadLibraryMaterial) of its own as well
MATERIAL_API = [
    ("ShadeViewRayHits", "RT64_ShadeViewRayHits", C.c_int, [_P, _P, _P, _P, _P, C.c_size_t]),
    ("ShadeViewRayHitsDevice", "RT64_ShadeViewRayHitsDevice", C.c_int, [_P, _P, _P, _P, _P, C.c_size_t, _P]),
    ("TraceViewRayMaterials", "RT64_TraceViewRayMaterials", C.c_int, [_P, _P, _P, _P, _P, C.c_size_t, C.c_uint]),
]
(MATERIAL_VALID, MATERIAL_BAD_HIT, MATERIAL_TEXTURED, MATERIAL_NORMAL_MAPPED, MATERIAL_SPECULAR_MAPPED, MATERIAL_CUTOUT, MATERIAL_SHADOW_CUTOUT,
 MATERIAL_NOISE_ALPHA, MATERIAL_BACK_FACE) = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20, 0x40, 0x80, 0x100
# include/rt64_alpha.h: walks that honour alpha (rules K1-K10), a list and a loader (RT64_LoadLibraryAlpha) of its own
ALPHA_API = [
    ("TraceViewRaysAlpha", "RT64_TraceViewRaysAlpha", C.c_int, [_P, _P, _P, _P, C.c_size_t, C.c_uint]),
    ("TraceViewRaysAlphaDevice", "RT64_TraceViewRaysAlphaDevice", C.c_int, [_P, _P, _P, _P, C.c_size_t, C.c_uint, _P]),
    ("TraceViewRayVisibility", "RT64_TraceViewRayVisibility", C.c_int, [_P, _P, _P, C.c_size_t, C.c_uint]),
    ("TraceViewRayVisibilityDevice", "RT64_TraceViewRayVisibilityDevice", C.c_int, [_P, _P, _P, C.c_size_t, C.c_uint, _P]),
]
VISIBILITY_VALID, VISIBILITY_BLOCKED = 0x1, 0x2
# include/rt64_lighting.h: direct-light records for hits (rules P1-P11), a list and a loader (RT64_LoadLibraryLighting) of its own
LIGHTING_API = [
    ("LightViewRayHits", "RT64_LightViewRayHits", C.c_int, [_P, _P, _P, _P, _P, C.c_size_t]),
    ("LightViewRayHitsDevice", "RT64_LightViewRayHitsDevice", C.c_int, [_P, _P, _P, _P, _P, C.c_size_t, _P]),
    ("TraceViewRayLighting", "RT64_TraceViewRayLighting", C.c_int, [_P, _P, _P, _P, _P, C.c_size_t, C.c_uint]),
]
LIGHTING_VALID, LIGHTING_BAD_HIT, LIGHTING_BACK_FACE, LIGHTING_UNLIT, LIGHTING_TRUNCATED = 0x01, 0x02, 0x04, 0x08, 0x10
# include/rt64_footprint.h: camera rays with differentials and texture footprints for hits (rules F1-F11), a list and a loader (RT64_LoadLibraryFootprint) of its own
FOOTPRINT_API = [
    ("GenerateViewCameraRays", "RT64_GenerateViewCameraRays", C.c_int, [_P, _P, _P, _P, C.c_size_t]),
    ("GenerateViewCameraRaysDevice", "RT64_GenerateViewCameraRaysDevice", C.c_int, [_P, _P, _P, _P, C.c_size_t, _P]),
    ("FootprintViewRayHits", "RT64_FootprintViewRayHits", C.c_int, [_P, _P, _P, _P, _P, C.c_size_t]),
    ("FootprintViewRayHitsDevice", "RT64_FootprintViewRayHitsDevice", C.c_int, [_P, _P, _P, _P, _P, C.c_size_t, _P]),
    ("TraceViewPixelFootprints", "RT64_TraceViewPixelFootprints", C.c_int, [_P, _P, _P, _P, _P, C.c_size_t, C.c_uint]),
]
FOOTPRINT_VALID, FOOTPRINT_BAD_HIT, FOOTPRINT_HAS_UV, FOOTPRINT_TEXTURED = 0x01, 0x02, 0x04, 0x08
# include/rt64_bounce.h: the frame's mirror and glass rays for hits, mirror chains (rules R1-R12), a list and a loader (RT64_LoadLibraryBounce) of its own
BOUNCE_API = [
    ("BounceViewRayHits", "RT64_BounceViewRayHits", C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.c_size_t]),
    ("BounceViewRayHitsDevice", "RT64_BounceViewRayHitsDevice", C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.c_size_t, _P]),
    ("TraceViewRayBounces", "RT64_TraceViewRayBounces", C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.c_size_t, C.c_uint]),
    ("TraceViewRayMirrorChains", "RT64_TraceViewRayMirrorChains", C.c_int, [_P, _P, _P, C.c_uint, _P, _P, C.c_size_t, C.c_uint]),
    ("TraceViewRayMirrorChainsDevice", "RT64_TraceViewRayMirrorChainsDevice", C.c_int, [_P, _P, _P, C.c_uint, _P, _P, C.c_size_t, C.c_uint, _P]),
]
(BOUNCE_VALID, BOUNCE_BAD_HIT, BOUNCE_BACK_FACE, BOUNCE_MIRROR, BOUNCE_GLASS, BOUNCE_TOTAL_INTERNAL, BOUNCE_CONTINUED) = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20, 0x40
MIRROR_CHAIN_MAX_DEPTH = 8
# include/rt64_layers.h: a ray's sorted hit list and each layer's weight (rules T1-T12), a list and a loader (RT64_LoadLibraryLayers) of its own
LAYERS_API = [
    ("TraceViewRayLayers", "RT64_TraceViewRayLayers", C.c_int, [_P, _P, _P, C.c_uint, _P, _P, _P, _P, C.c_size_t, C.c_uint]),
    ("TraceViewRayLayersDevice", "RT64_TraceViewRayLayersDevice", C.c_int, [_P, _P, _P, C.c_uint, _P, _P, C.c_size_t, C.c_uint, _P]),
    ("WeighViewRayLayers", "RT64_WeighViewRayLayers", C.c_int, [_P, _P, _P, _P, C.c_uint, _P, _P, C.c_size_t]),
    ("WeighViewRayLayersDevice", "RT64_WeighViewRayLayersDevice", C.c_int, [_P, _P, _P, _P, C.c_uint, _P, _P, C.c_size_t, _P]),
]
LAYERS_VALID, LAYERS_ENDS_OPAQUE, LAYERS_FULL = 0x1, 0x2, 0x4
COVERAGE_VALID, COVERAGE_COVERED, COVERAGE_GLASS, COVERAGE_BAD_HIT = 0x1, 0x2, 0x4, 0x8
RAY_LAYERS_MAX = 16
# include/rt64_sampled_lighting.h: the direct light of a hit as a frame's pixel samples it (rules J1-J11), a list and a loader (RT64_LoadLibrarySampledLighting) of its own
SAMPLED_LIGHTING_API = [
    ("SampleViewRayLights", "RT64_SampleViewRayLights", C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.c_size_t]),
    ("SampleViewRayLightsDevice", "RT64_SampleViewRayLightsDevice", C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.c_size_t, _P]),
    ("TraceViewRaySampledLights", "RT64_TraceViewRaySampledLights", C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.c_size_t, C.c_uint]),
]
(SAMPLED_LIGHTING_VALID, SAMPLED_LIGHTING_BAD_HIT, SAMPLED_LIGHTING_BACK_FACE, SAMPLED_LIGHTING_UNLIT, SAMPLED_LIGHTING_TRUNCATED) = 0x01, 0x02, 0x04, 0x08, 0x10
LIGHT_SAMPLING_MAX_LIGHTS, LIGHT_SAMPLING_MAX_SAMPLES = 16, 64
# include/rt64_indirect.h: the indirect light of a point as a frame's pixel samples it (rules Y1-Y12), a list and a loader (RT64_LoadLibraryIndirect) of its own
INDIRECT_API = [
    ("GenerateViewPointGIRays", "RT64_GenerateViewPointGIRays", C.c_int, [_P, _P, _P, _P, C.c_uint, C.c_uint, _P, C.c_size_t]),
    ("GenerateViewPointGIRaysDevice", "RT64_GenerateViewPointGIRaysDevice", C.c_int, [_P, _P, _P, _P, C.c_uint, C.c_uint, _P, C.c_size_t, _P]),
    ("ComposeViewGIRays", "RT64_ComposeViewGIRays", C.c_int, [_P, _P, _P, C.c_uint, _P, _P, _P, _P, C.c_size_t]),
    ("ComposeViewGIRaysDevice", "RT64_ComposeViewGIRaysDevice", C.c_int, [_P, _P, _P, C.c_uint, _P, _P, _P, _P, C.c_size_t, _P]),
    ("TraceViewPointsIndirect", "RT64_TraceViewPointsIndirect", C.c_int, [_P, _P, _P, _P, _P, _P, C.c_size_t]),
    ("TraceViewPointsIndirectDevice", "RT64_TraceViewPointsIndirectDevice", C.c_int, [_P, _P, _P, _P, _P, _P, C.c_size_t, _P]),
    ("TraceViewRayIndirect", "RT64_TraceViewRayIndirect", C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.c_size_t, C.c_uint]),
]
GI_POINT_NONE, GI_RAYS_SECOND_BOUNCE = 0x1, 0x1
(GI_SAMPLE_VALID, GI_SAMPLE_BAD_HIT, GI_SAMPLE_SURFACE, GI_SAMPLE_COVERED, GI_SAMPLE_UNLIT, GI_SAMPLE_TRUNCATED) = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20
INDIRECT_VALID, INDIRECT_BAD_POINT, INDIRECT_BAD_HIT = 0x1, 0x2, 0x4
GI_SAMPLING_MAX_SAMPLES, GI_SAMPLING_MAX_BOUNCES = 64, 2
# include/rt64_radiance.h: the colour a ray brings back and the sky behind it (rules W1-W12), a list and a loader (RT64_LoadLibraryRadiance) of its own
RADIANCE_API = [
    ("SkyViewRays", "RT64_SkyViewRays", C.c_int, [_P, _P, _P, C.c_size_t]),
    ("SkyViewRaysDevice", "RT64_SkyViewRaysDevice", C.c_int, [_P, _P, _P, C.c_size_t, _P]),
    ("SkyViewPixels", "RT64_SkyViewPixels", C.c_int, [_P, _P, _P, C.c_size_t]),
    ("SkyViewPixelsDevice", "RT64_SkyViewPixelsDevice", C.c_int, [_P, _P, _P, C.c_size_t, _P]),
    ("ComposeViewRayRadiance", "RT64_ComposeViewRayRadiance", C.c_int, [_P, _P, _P, _P, C.c_uint, _P, C.c_size_t, C.c_uint]),
    ("ComposeViewRayRadianceDevice", "RT64_ComposeViewRayRadianceDevice", C.c_int, [_P, _P, _P, _P, C.c_uint, _P, C.c_size_t, C.c_uint, _P]),
    ("TraceViewRayRadiance", "RT64_TraceViewRayRadiance", C.c_int, [_P, _P, _P, C.c_uint, _P, _P, _P, C.c_size_t, C.c_uint]),
]
SKY_VALID, SKY_NO_TEXTURE, SKY_BACKGROUND = 0x1, 0x2, 0x4
(RADIANCE_VALID, RADIANCE_COVERED, RADIANCE_BAD_HIT, RADIANCE_LIT, RADIANCE_FOGGED, RADIANCE_TRUNCATED) = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20
RADIANCE_FLAG_UNSHADOWED, RADIANCE_FLAG_FOG_FROM_CAMERA = 0x100, 0x200


class RAY(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("tMin", C.c_float), ("direction", C.c_float * 3), ("tMax", C.c_float)]


class RAY_HIT(C.Structure):
    _fields_ = [("t", C.c_float), ("u", C.c_float), ("v", C.c_float), ("instance", C.c_int), ("primitive", C.c_uint),
                ("nodesVisited", C.c_uint), ("trianglesTested", C.c_uint), ("reserved", C.c_uint)]


class RAY_SURFACE(C.Structure):
    _fields_ = [("position", C.c_float * 3), ("flags", C.c_uint), ("geometricNormal", C.c_float * 3), ("instance", C.c_int),
                ("shadingNormal", C.c_float * 3), ("primitive", C.c_uint), ("uv", C.c_float * 2), ("t", C.c_float), ("reserved", C.c_uint)]


class RAY_MATERIAL(C.Structure):
    _fields_ = [("color", C.c_float * 4), ("shadingNormal", C.c_float * 3), ("flags", C.c_uint), ("specular", C.c_float * 3), ("shadowAlpha", C.c_float),
                ("lod", C.c_float), ("instance", C.c_int), ("primitive", C.c_uint), ("reserved", C.c_uint)]


class RAY_VISIBILITY(C.Structure):
    _fields_ = [("visibility", C.c_float), ("flags", C.c_uint), ("nodesVisited", C.c_uint), ("trianglesTested", C.c_uint)]


class RAY_LIGHTING(C.Structure):
    _fields_ = [("direct", C.c_float * 3), ("flags", C.c_uint), ("unshadowed", C.c_float * 3), ("lightsAdmitted", C.c_uint),
                ("emitted", C.c_float * 3), ("lightsBlocked", C.c_uint), ("instance", C.c_int), ("primitive", C.c_uint),
                ("nodesVisited", C.c_uint), ("trianglesTested", C.c_uint)]


class LIGHT_SAMPLE_KEY(C.Structure):
    _fields_ = [("x", C.c_uint), ("y", C.c_uint), ("frame", C.c_uint), ("reserved", C.c_uint)]


class LIGHT_SAMPLING(C.Structure):
    _fields_ = [("maxLights", C.c_int), ("diSamples", C.c_int), ("flags", C.c_uint), ("reserved", C.c_uint)]


class RAY_SAMPLED_LIGHTING(C.Structure):
    _fields_ = [("direct", C.c_float * 3), ("flags", C.c_uint), ("unshadowed", C.c_float * 3), ("lightsAdmitted", C.c_uint),
                ("emitted", C.c_float * 3), ("drawn", C.c_uint), ("instance", C.c_int), ("primitive", C.c_uint),
                ("nodesVisited", C.c_uint), ("trianglesTested", C.c_uint)]


class RAY_DIFFERENTIAL(C.Structure):
    _fields_ = [("dOdx", C.c_float * 3), ("reserved0", C.c_uint), ("dOdy", C.c_float * 3), ("reserved1", C.c_uint),
                ("dDdx", C.c_float * 3), ("reserved2", C.c_uint), ("dDdy", C.c_float * 3), ("reserved3", C.c_uint)]


class RAY_FOOTPRINT(C.Structure):
    _fields_ = [("duvdx", C.c_float * 2), ("duvdy", C.c_float * 2), ("lod", C.c_float), ("lodNormal", C.c_float), ("lodSpecular", C.c_float),
                ("flags", C.c_uint), ("dPdx", C.c_float * 3), ("instance", C.c_int), ("dPdy", C.c_float * 3), ("primitive", C.c_uint)]


class RAY_BOUNCE(C.Structure):
    _fields_ = [("fresnel", C.c_float), ("reflectionFactor", C.c_float), ("refractionFactor", C.c_float), ("flags", C.c_uint),
                ("instance", C.c_int), ("primitive", C.c_uint), ("nodesVisited", C.c_uint), ("trianglesTested", C.c_uint)]


class RAY_LAYERS(C.Structure):
    _fields_ = [("count", C.c_uint), ("flags", C.c_uint), ("nodesVisited", C.c_uint), ("trianglesTested", C.c_uint)]


class RAY_COVERAGE(C.Structure):
    _fields_ = [("transmittance", C.c_float), ("refraction", C.c_float), ("shaded", C.c_uint), ("flags", C.c_uint)]


class RAY_SKY(C.Structure):
    _fields_ = [("color", C.c_float * 3), ("alpha", C.c_float), ("uv", C.c_float * 2), ("flags", C.c_uint), ("reserved", C.c_uint)]


class RAY_RADIANCE(C.Structure):
    _fields_ = [("radiance", C.c_float * 3), ("flags", C.c_uint), ("surface", C.c_float * 3), ("transmittance", C.c_float),
                ("transparent", C.c_float * 3), ("litLayer", C.c_int), ("light", C.c_float * 3), ("layers", C.c_uint)]


class GI_POINT(C.Structure):
    _fields_ = [("position", C.c_float * 3), ("flags", C.c_uint), ("normal", C.c_float * 3), ("instance", C.c_int)]


class GI_SAMPLING(C.Structure):
    _fields_ = [("giSamples", C.c_int), ("giBounces", C.c_int), ("diSamples", C.c_int), ("flags", C.c_uint)]


class GI_SAMPLE(C.Structure):
    _fields_ = [("radiance", C.c_float * 3), ("remaining", C.c_float), ("position", C.c_float * 3), ("flags", C.c_uint), ("normal", C.c_float * 3), ("instance", C.c_int),
                ("layers", C.c_uint), ("reserved", C.c_uint), ("nodesVisited", C.c_uint), ("trianglesTested", C.c_uint)]


class POINT_INDIRECT(C.Structure):
    _fields_ = [("indirect", C.c_float * 3), ("samples", C.c_float), ("moments", C.c_float * 2), ("flags", C.c_uint), ("instance", C.c_int),
                ("rays", C.c_uint), ("nodesVisited", C.c_uint), ("trianglesTested", C.c_uint), ("reserved", C.c_uint)]


assert C.sizeof(RAY_LAYERS) == 16 and C.sizeof(RAY_COVERAGE) == 16
assert C.sizeof(GI_POINT) == 32 and C.sizeof(GI_SAMPLING) == 16 and C.sizeof(GI_SAMPLE) == 64 and C.sizeof(POINT_INDIRECT) == 48
assert C.sizeof(LIGHT_SAMPLE_KEY) == 16 and C.sizeof(LIGHT_SAMPLING) == 16 and C.sizeof(RAY_SAMPLED_LIGHTING) == 64
assert C.sizeof(RAY_SKY) == 32 and C.sizeof(RAY_RADIANCE) == 64
assert C.sizeof(RAY_VISIBILITY) == 16 and C.sizeof(RAY_LIGHTING) == 64 and C.sizeof(RAY_BOUNCE) == 32
assert C.sizeof(RAY_DIFFERENTIAL) == 64 and C.sizeof(RAY_FOOTPRINT) == 64
assert C.sizeof(RAY) == 32 and C.sizeof(RAY_HIT) == 32 and C.sizeof(RAY_SURFACE) == 64 and C.sizeof(RAY_MATERIAL) == 64

HALO_ROWS = 62
HALO_BYTES_PER_PIXEL = 24


class HALO_REGION(C.Structure):
    _fields_ = [("peer", C.c_int), ("send", C.c_int), ("y0", C.c_int), ("y1", C.c_int), ("host", C.c_void_p), ("bytes", C.c_size_t)]


HALO_EXCHANGE = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(HALO_REGION), C.c_int)
GATHER_ID_BYTES = 128


class Library:
    """RT64_LoadLibrary(): dlopen + one dlsym per table member.  Members are attributes (lib.CreateDevice ...)."""

    def __init__(self, path=None):
        path = path or os.environ.get("RT64_LIBRARY_PATH") or DEFAULT_LIBRARY
        if not os.path.exists(path):
            raise FileNotFoundError(
                f"{path} not found: the HIP library is not built (run `python -c 'import __graft_entry__ as g; g.build()'`). "
                "There is no CPU fallback.")
        self.path = path
        self.handle = C.CDLL(path, mode=C.RTLD_LOCAL)
        for member, symbol, restype, argtypes in API + EXT_API + QUERY_API + SURFACE_API + MATERIAL_API + ALPHA_API + LIGHTING_API + SAMPLED_LIGHTING_API + FOOTPRINT_API + BOUNCE_API + LAYERS_API + RADIANCE_API + INDIRECT_API:
            fn = getattr(self.handle, symbol)      # AttributeError if an export is missing
            fn.restype = restype
            fn.argtypes = argtypes
            setattr(self, member, fn)

    def last_error(self):
        e = self.GetLastError()
        return e.decode() if e else ""


def exported_symbols():
    """Every symbol include/rt64.h declares (33 reference exports + extensions)."""
    return [s for _, s, _, _ in API + EXT_API]


class _Scalar:
    """An argument of a query entry point that is a plain number between its arrays (_query's kind "value")."""
    def __init__(self, value):
        self.value = value


def _out_shape(n, width):
    """(N, width), or (segments, N, width) for a width given as (segments, width): a chain's segment-major records."""
    return (width[0], n, width[1]) if isinstance(width, tuple) else (n, width)


def _query(lib, view, host, device, args, flags=None, stream=None):
    """The call behind every ray-query wrapper.  `args` lists the entry point's array arguments in its order as (kind, value) pairs: ("in", an (N, 8)
    float32 array: rays, hits), ("lods", an (N,) float32 array, or None for NULL), ("diffs", an (N, 16) float32 array of RT64_RAY_DIFFERENTIALs, or None for
    NULL), ("out", the width of an (N, width) float32 array to allocate -- None: NULL, nothing is returned for it; (S, width): an (S, N, width) array), ("value", a
    number passed as it is).
    NumPy inputs go to the entry point `host`; torch tensors to `device` (None: the call has no device form), enqueued on `stream`.  Behind the
    arrays go count, flags (unless None) and the stream.  Returns the outputs in order; raises ValueError for a wrong array,
    RuntimeError(RT64_GetLastError) on a refusal."""
    ins = [v for kind, v in args if kind == "in"]
    lods = next((v for kind, v in args if kind == "lods"), None)
    diffs = next((v for kind, v in args if kind == "diffs"), None)
    on_device = device is not None and type(ins[0]).__module__.split(".")[0] == "torch"
    if on_device:
        import torch
        for a in ins:
            if a.dim() != 2 or a.shape[1] != 8 or a.dtype != torch.float32 or not a.is_cuda:
                raise ValueError("rays: an (N, 8) float32 CUDA tensor" if len(ins) == 1 else "rays, hits: (N, 8) float32 CUDA tensors")
        if any(a.shape[0] != ins[0].shape[0] for a in ins):
            raise ValueError("one hit per ray")
        if lods is not None and (lods.dim() != 1 or lods.shape[0] != ins[0].shape[0] or lods.dtype != torch.float32 or not lods.is_cuda):
            raise ValueError("lods: an (N,) float32 CUDA tensor")
        if diffs is not None and (diffs.dim() != 2 or tuple(diffs.shape) != (ins[0].shape[0], 16) or diffs.dtype != torch.float32 or not diffs.is_cuda):
            raise ValueError("diffs: an (N, 16) float32 CUDA tensor")
        ins, lods = [a.contiguous() for a in ins], lods.contiguous() if lods is not None else None
        diffs = diffs.contiguous() if diffs is not None else None
        new = lambda width: torch.empty(_out_shape(ins[0].shape[0], width), dtype=torch.float32, device=ins[0].device)
        address = lambda a: a.data_ptr()
    else:
        import numpy as np
        ins = [np.ascontiguousarray(a, dtype=np.float32) for a in ins]
        if ins[0].ndim != 2 or ins[0].shape[1] != 8 or any(a.shape != ins[0].shape for a in ins):
            raise ValueError("rays: an (N, 8) float32 array" if len(ins) == 1 else "rays, hits: (N, 8) float32 arrays of one length")
        if lods is not None:
            lods = np.ascontiguousarray(lods, dtype=np.float32)
            if lods.shape != (ins[0].shape[0],):
                raise ValueError("lods: an (N,) float32 array")
        if diffs is not None:
            diffs = np.ascontiguousarray(diffs, dtype=np.float32)
            if diffs.shape != (ins[0].shape[0], 16):
                raise ValueError("diffs: an (N, 16) float32 array")
        new = lambda width: np.empty(_out_shape(ins[0].shape[0], width), dtype=np.float32)
        address = lambda a: a.ctypes.data
    checked = iter(ins)
    arrays = [next(checked) if kind == "in" else lods if kind == "lods" else diffs if kind == "diffs" else _Scalar(v) if kind == "value" else new(v) if v is not None else None
              for kind, v in args]          # the entry point's arguments in front of count, in its order
    outs = [a for (kind, _), a in zip(args, arrays) if kind == "out" and a is not None]
    tail = []
    if on_device:
        s = stream if stream is not None else torch.cuda.current_stream(ins[0].device)
        if s != torch.cuda.current_stream(ins[0].device):
            for a in arrays:          # (the allocator must not hand the memory out again before the query has run)
                if a is not None and not isinstance(a, _Scalar):
                    a.record_stream(s)
        tail = [s.cuda_stream]
    pointers = [a.value if isinstance(a, _Scalar) else address(a) if a is not None else None for a in arrays]
    if not getattr(lib, device if on_device else host)(view, *pointers, ins[0].shape[0], *([] if flags is None else [flags]), *tail):
        raise RuntimeError(lib.last_error())
    return outs[0] if len(outs) == 1 else tuple(outs)


def trace_rays(lib, view, rays, flags=0, stream=None):
    """RT64_TraceViewRays on an (N, 8) float32 array of RT64_RAYs: origin xyz, tMin, direction xyz, tMax.

    A NumPy array takes the host path; a torch CUDA tensor the device path, enqueued on `stream` (a torch stream; default the tensor's
    current stream) behind the view's last frame.  Returns (N, 8) float32 hits of the same kind -- t, u, v, then instance, primitive,
    nodesVisited, trianglesTested, reserved as int32 / uint32 bits (read them through `.view(int32)`).  Raises with RT64_GetLastError on a refusal."""
    return _query(lib, view, "TraceViewRays", "TraceViewRaysDevice", [("in", rays), ("out", 8)], flags, stream)


def resolve_hits(lib, view, rays, hits, stream=None):
    """RT64_ResolveViewRayHits: (N, 8) float32 rays and the (N, 8) float32 hits trace_rays returned for them -> (N, 16) float32 RT64_RAY_SURFACEs:
    position xyz, flags, geometricNormal xyz, instance, shadingNormal xyz, primitive, uv, t, reserved (flags, instance, primitive as uint32 / int32
    bits: read them through `.view(int32)`).  NumPy arrays take the host path; torch CUDA tensors the device path, enqueued on `stream` like trace_rays."""
    return _query(lib, view, "ResolveViewRayHits", "ResolveViewRayHitsDevice", [("in", rays), ("in", hits), ("out", 16)], None, stream)


def trace_surfaces(lib, view, rays, flags=0):
    """RT64_TraceViewRaySurfaces on an (N, 8) float32 NumPy array of rays: trace and resolve in one staging round trip -> (hits (N, 8), surfaces (N, 16))."""
    return _query(lib, view, "TraceViewRaySurfaces", None, [("in", rays), ("out", 8), ("out", 16)], flags)


def shade_hits(lib, view, rays, hits, lods=None, stream=None):
    """RT64_ShadeViewRayHits: (N, 8) float32 rays, the (N, 8) float32 hits trace_rays returned for them and, optionally, (N,) float32 lods
    (None: level 0 for every record) -> (N, 16) float32 RT64_RAY_MATERIALs: color rgba, shadingNormal xyz, flags, specular xyz, shadowAlpha,
    lod, instance, primitive, reserved (flags, instance, primitive as uint32 / int32 bits: read them through `.view(int32)`).  NumPy arrays
    take the host path; torch CUDA tensors the device path, enqueued on `stream` like trace_rays."""
    return _query(lib, view, "ShadeViewRayHits", "ShadeViewRayHitsDevice", [("in", rays), ("in", hits), ("lods", lods), ("out", 16)], None, stream)


def trace_materials(lib, view, rays, lods=None, flags=0):
    """RT64_TraceViewRayMaterials on an (N, 8) float32 NumPy array of rays (and optional (N,) float32 lods): trace and shade in one staging
    round trip -> (hits (N, 8), materials (N, 16))."""
    return _query(lib, view, "TraceViewRayMaterials", None, [("in", rays), ("out", 8), ("lods", lods), ("out", 16)], flags)


def trace_rays_alpha(lib, view, rays, lods=None, flags=0, stream=None):
    """RT64_TraceViewRaysAlpha: (N, 8) float32 rays and, optionally, (N,) float32 lods (None: level 0 for every ray) -> (N, 8) float32 hits as
    trace_rays returns them, the closest intersection a texture-edge shader does not cut out (rule K2).  NumPy arrays take the host path; torch
    CUDA tensors the device path, enqueued on `stream` like trace_rays."""
    return _query(lib, view, "TraceViewRaysAlpha", "TraceViewRaysAlphaDevice", [("in", rays), ("lods", lods), ("out", 8)], flags, stream)


def trace_visibility(lib, view, rays, flags=0, stream=None):
    """RT64_TraceViewRayVisibility: (N, 8) float32 rays -> (N, 4) float32 RT64_RAY_VISIBILITYs: visibility, then flags, nodesVisited, trianglesTested
    as uint32 bits (read them through `.view(int32)`): what a frame's shadow ray returns for the ray, noise aside (rule K5).  NumPy arrays take the
    host path; torch CUDA tensors the device path, enqueued on `stream` like trace_rays."""
    return _query(lib, view, "TraceViewRayVisibility", "TraceViewRayVisibilityDevice", [("in", rays), ("out", 4)], flags, stream)


def light_hits(lib, view, rays, hits, lods=None, stream=None):
    """RT64_LightViewRayHits: (N, 8) float32 rays, the (N, 8) float32 hits a trace returned for them and, optionally, (N,) float32 lods (None: level 0
    for every record) -> (N, 16) float32 RT64_RAY_LIGHTINGs: direct rgb, flags, unshadowed rgb, lightsAdmitted, emitted rgb, lightsBlocked, then
    instance, primitive, nodesVisited, trianglesTested (the integers as uint32 / int32 bits: read them through `.view(int32)`): the direct light of
    the view's last frame at each hit, every admitted light once at its centre (rules P1-P11).  NumPy arrays take the host path; torch CUDA tensors
    the device path, enqueued on `stream` like trace_rays."""
    return _query(lib, view, "LightViewRayHits", "LightViewRayHitsDevice", [("in", rays), ("in", hits), ("lods", lods), ("out", 16)], None, stream)


def trace_lighting(lib, view, rays, lods=None, flags=0):
    """RT64_TraceViewRayLighting on an (N, 8) float32 NumPy array of rays (and optional (N,) float32 lods): the walk of trace_rays_alpha and the
    records of light_hits in one staging round trip -> (hits (N, 8), lighting (N, 16)).  `flags`: RAY_FLAG_CULL_BACK_FACING only."""
    return _query(lib, view, "TraceViewRayLighting", None, [("in", rays), ("out", 8), ("lods", lods), ("out", 16)], flags)


LIGHT_SAMPLE_KEY_DTYPE = [("x", "<u4"), ("y", "<u4"), ("frame", "<u4"), ("reserved", "<u4")]          # numpy dtypes of the three structs of rt64_sampled_lighting.h
LIGHT_SAMPLING_DTYPE = [("maxLights", "<i4"), ("diSamples", "<i4"), ("flags", "<u4"), ("reserved", "<u4")]
RAY_SAMPLED_LIGHTING_DTYPE = [("direct", "<f4", (3,)), ("flags", "<u4"), ("unshadowed", "<f4", (3,)), ("lightsAdmitted", "<u4"), ("emitted", "<f4", (3,)), ("drawn", "<u4"),
                              ("instance", "<i4"), ("primitive", "<u4"), ("nodesVisited", "<u4"), ("trianglesTested", "<u4")]


def _sample_keys(rays, keys, stream):
    """The keys argument of the sampled-lighting wrappers -> (address or None, the array to keep alive): an (N, 4) uint32 array of RT64_LIGHT_SAMPLE_KEYs (x, y, frame,
    reserved; a structured array of LIGHT_SAMPLE_KEY_DTYPE as well) of the kind the rays are, or None for NULL."""
    if keys is None:
        return None, None
    n = rays.shape[0] if hasattr(rays, "shape") and len(rays.shape) else -1
    if type(rays).__module__.split(".")[0] == "torch":
        import torch
        if type(keys).__module__.split(".")[0] != "torch" or keys.dim() != 2 or tuple(keys.shape) != (n, 4) or keys.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)) or not keys.is_cuda:
            raise ValueError("keys: an (N, 4) int32 or uint32 CUDA tensor")
        keys = keys.contiguous()
        s = stream if stream is not None else torch.cuda.current_stream(keys.device)
        if s != torch.cuda.current_stream(keys.device):
            keys.record_stream(s)
        return keys.data_ptr(), keys
    import numpy as np
    keys = np.asarray(keys)
    if keys.dtype.names is not None:
        keys = np.ascontiguousarray(keys, dtype=np.dtype(LIGHT_SAMPLE_KEY_DTYPE)).view(np.uint32).reshape(-1, 4)
    if keys.ndim != 2 or keys.shape != (n, 4) or keys.dtype.kind not in "iu":
        raise ValueError("keys: an (N, 4) uint32 array")
    keys = np.ascontiguousarray(keys.astype(np.uint32, copy=False))
    return keys.ctypes.data, keys


def _light_sampling(max_lights, di_samples):
    """RT64_LIGHT_SAMPLING of the two overrides (-1: the last frame's value) -> (address or None for NULL, the struct to keep alive)."""
    if max_lights == -1 and di_samples == -1:
        return None, None
    s = LIGHT_SAMPLING(int(max_lights), int(di_samples), 0, 0)
    return C.addressof(s), s


def sample_lighting(lib, view, rays, hits, lods=None, keys=None, max_lights=-1, di_samples=-1, stream=None):
    """RT64_SampleViewRayLights: (N, 8) float32 rays, the (N, 8) float32 hits a trace returned for them, optionally (N,) float32 lods (None: level 0) and (N, 4)
    uint32 keys (x, y, frame, reserved; None: record i is keyed as pixel i of the last frame, row by row, at its frame count) -> (N, 16) float32
    RT64_RAY_SAMPLED_LIGHTINGs: direct rgb, flags, unshadowed rgb, lightsAdmitted, emitted rgb, drawn, then instance, primitive, nodesVisited, trianglesTested (the
    integers as uint32 / int32 bits: read them through `.view(int32)`, or the whole array through `.view(RAY_SAMPLED_LIGHTING_DTYPE)`): the direct light of the view's
    last frame at each hit as the pixel of the key samples it (rules J1-J11).  `max_lights` (0 .. 16) and `di_samples` (0 .. 64) override the frame's values; -1 keeps
    them.  NumPy arrays take the host path; torch CUDA tensors the device path, enqueued on `stream` like trace_rays."""
    k, keep_k = _sample_keys(rays, keys, stream)
    p, keep_p = _light_sampling(max_lights, di_samples)
    return _query(lib, view, "SampleViewRayLights", "SampleViewRayLightsDevice", [("in", rays), ("in", hits), ("lods", lods), ("value", k), ("value", p), ("out", 16)], None, stream)


def trace_sampled_lighting(lib, view, rays, lods=None, keys=None, max_lights=-1, di_samples=-1, flags=0):
    """RT64_TraceViewRaySampledLights on an (N, 8) float32 NumPy array of rays (optional (N,) float32 lods and (N, 4) uint32 keys): the walk of trace_rays_alpha and
    the records of sample_lighting in one staging round trip -> (hits (N, 8), records (N, 16)).  `flags`: RAY_FLAG_CULL_BACK_FACING only."""
    k, keep_k = _sample_keys(rays, keys, None)
    p, keep_p = _light_sampling(max_lights, di_samples)
    return _query(lib, view, "TraceViewRaySampledLights", None, [("in", rays), ("out", 8), ("lods", lods), ("value", k), ("value", p), ("out", 16)], flags)


def _pixel_query(lib, view, host, device, pixels, count, widths, flags=None, stream=None):
    """_query's sibling for the calls that start from pixels: `pixels` is an (N, 2) uint32 array of (x, y) pairs -- NumPy: the entry point `host`; a torch CUDA tensor
    (int32 or uint32 bits): `device`, enqueued on `stream` -- or None with `count`: the first `count` pixels of the frame row by row, on the host path unless `stream`
    (a torch stream) names the device one.  `widths` lists the outputs in the entry point's order: the width of an (N, width) float32 array to allocate, or None for
    NULL.  Returns the allocated outputs in order."""
    on_device = device is not None and (type(pixels).__module__.split(".")[0] == "torch" or (pixels is None and stream is not None))
    if pixels is None:
        if count is None or int(count) < 0:
            raise ValueError("pixels=None needs a count")
        n = int(count)
    elif count is not None:
        raise ValueError("count goes with pixels=None only")
    if on_device:
        import torch
        if pixels is not None:
            if pixels.dim() != 2 or pixels.shape[1] != 2 or pixels.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)) or not pixels.is_cuda:
                raise ValueError("pixels: an (N, 2) uint32 / int32 CUDA tensor")
            pixels = pixels.contiguous()
            n, where = pixels.shape[0], pixels.device
        else:
            where = torch.device("cuda", torch.cuda.current_device())
        new = lambda width: torch.empty((n, width), dtype=torch.float32, device=where)
        address = lambda a: a.data_ptr()
    else:
        import numpy as np
        if pixels is not None:
            pixels = np.ascontiguousarray(pixels, dtype=np.uint32)
            if pixels.ndim != 2 or pixels.shape[1] != 2:
                raise ValueError("pixels: an (N, 2) uint32 array")
            n = pixels.shape[0]
        new = lambda width: np.empty((n, width), dtype=np.float32)
        address = lambda a: a.ctypes.data
    outs = [new(w) if w is not None else None for w in widths]
    tail = []
    if on_device:
        s = stream if stream is not None else torch.cuda.current_stream(where)
        if s != torch.cuda.current_stream(where):
            for a in [pixels] + outs:          # (the allocator must not hand the memory out again before the query has run)
                if a is not None:
                    a.record_stream(s)
        tail = [s.cuda_stream]
    pointers = [address(a) if a is not None else None for a in [pixels] + outs]
    if not getattr(lib, device if on_device else host)(view, *pointers, n, *([] if flags is None else [flags]), *tail):
        raise RuntimeError(lib.last_error())
    outs = [a for a in outs if a is not None]
    return outs[0] if len(outs) == 1 else tuple(outs)


def camera_rays(lib, view, pixels=None, count=None, differentials=True, stream=None):
    """RT64_GenerateViewCameraRays: the camera rays the view's last frame traced for `pixels` -- an (N, 2) uint32 array of (x, y), or None with `count`: the frame's
    first `count` pixels row by row -- as (N, 8) float32 RT64_RAYs (that frame's jitter included, direction not normalised, tMin 0.1, tMax 100000) and, with
    `differentials`, their (N, 16) float32 RT64_RAY_DIFFERENTIALs: dOdx xyz, reserved, dOdy xyz, reserved, dDdx xyz, reserved, dDdy xyz, reserved (rules F1-F3).
    Returns rays, or (rays, diffs).  A NumPy array takes the host path; a torch CUDA tensor the device path, enqueued on `stream` like trace_rays."""
    return _pixel_query(lib, view, "GenerateViewCameraRays", "GenerateViewCameraRaysDevice", pixels, count, [8, 16 if differentials else None], None, stream)


def footprint_hits(lib, view, rays, diffs, hits, stream=None):
    """RT64_FootprintViewRayHits: (N, 8) float32 rays, their (N, 16) float32 differentials (None: all 0, what a frame's secondary rays carry) and the (N, 8) float32
    hits a trace returned for them -> (N, 16) float32 RT64_RAY_FOOTPRINTs: duvdx xy, duvdy xy, lod, lodNormal, lodSpecular, flags, dPdx xyz, instance, dPdy xyz,
    primitive (flags, instance, primitive as uint32 / int32 bits: read them through `.view(int32)`): the UV gradients and the clamped mip levels the frame's
    surface any-hit program uses for the hit (rules F4-F8).  NumPy arrays take the host path; torch CUDA tensors the device path, enqueued on `stream` like trace_rays."""
    return _query(lib, view, "FootprintViewRayHits", "FootprintViewRayHitsDevice", [("in", rays), ("diffs", diffs), ("in", hits), ("out", 16)], None, stream)


def trace_pixel_footprints(lib, view, pixels=None, count=None, flags=0):
    """RT64_TraceViewPixelFootprints on an (N, 2) uint32 NumPy array of pixels (or None with `count`): camera_rays, the walk of trace_rays and footprint_hits in one
    staging round trip -> (rays (N, 8), hits (N, 8), footprints (N, 16)).  `flags`: RAY_FLAG_CULL_BACK_FACING only."""
    return _pixel_query(lib, view, "TraceViewPixelFootprints", None, pixels, count, [8, 8, 16], flags)


def bounce_view_ray_hits(lib, view, rays, hits, lods=None, bounces=True, reflected=True, refracted=True, stream=None):
    """RT64_BounceViewRayHits: (N, 8) float32 rays, the (N, 8) float32 hits a trace returned for them and, optionally, (N,) float32 lods (None: level 0 for every
    record) -> (N, 8) float32 RT64_RAY_BOUNCEs (fresnel, reflectionFactor, refractionFactor, then flags, instance, primitive, nodesVisited, trianglesTested as uint32 /
    int32 bits: read them through `.view(int32)`), the (N, 8) reflected RT64_RAYs and the (N, 8) refracted RT64_RAYs: the rays a frame's reflection and refraction
    passes cast from each hit (rules R1-R6).  `bounces`, `reflected`, `refracted` = False passes NULL for that output and leaves it out of the result; not all three.
    NumPy arrays take the host path; torch CUDA tensors the device path, enqueued on `stream` like trace_rays."""
    return _query(lib, view, "BounceViewRayHits", "BounceViewRayHitsDevice",
                  [("in", rays), ("in", hits), ("lods", lods), ("out", 8 if bounces else None), ("out", 8 if reflected else None), ("out", 8 if refracted else None)], None, stream)


def trace_view_ray_bounces(lib, view, rays, lods=None, flags=0, bounces=True, reflected=True, refracted=True):
    """RT64_TraceViewRayBounces on an (N, 8) float32 NumPy array of rays (and optional (N,) float32 lods): the walk of trace_rays_alpha and the records of
    bounce_view_ray_hits in one staging round trip -> (hits (N, 8), bounces (N, 8), reflected (N, 8), refracted (N, 8)), without the outputs switched off."""
    return _query(lib, view, "TraceViewRayBounces", None,
                  [("in", rays), ("out", 8), ("lods", lods), ("out", 8 if bounces else None), ("out", 8 if reflected else None), ("out", 8 if refracted else None)], flags)


def trace_view_ray_mirror_chains(lib, view, rays, depth, lods=None, flags=0, stream=None):
    """RT64_TraceViewRayMirrorChains: (N, 8) float32 rays and, optionally, (N,) float32 lods -> (hits (depth, N, 8), bounces (depth, N, 8)): segment 0 is the walk of
    trace_rays_alpha, every later segment the walk of the previous segment's reflected ray at lod 0 while the hit is a mirror (rule R7); 1 <= depth <= 8.  `flags`:
    RAY_FLAG_CULL_BACK_FACING only.  NumPy arrays take the host path; torch CUDA tensors the device path, enqueued on `stream` like trace_rays."""
    depth = int(depth)
    return _query(lib, view, "TraceViewRayMirrorChains", "TraceViewRayMirrorChainsDevice",
                  [("in", rays), ("lods", lods), ("value", depth), ("out", (max(depth, 0), 8)), ("out", (max(depth, 0), 8))], flags, stream)


def _is_torch(a):
    return type(a).__module__.split(".")[0] == "torch"


def _as_uint32(a):
    """The uint32 bits of a float32 output array (NumPy: a view; torch: int32 where the build has no uint32)."""
    if _is_torch(a):
        import torch
        return a.view(getattr(torch, "uint32", torch.int32))
    import numpy as np
    return a.view(np.uint32)


def _layer_count(max_layers):
    max_layers = int(max_layers)
    if not 1 <= max_layers <= RAY_LAYERS_MAX:
        raise ValueError("max_layers: 1 to %d" % RAY_LAYERS_MAX)
    return max_layers


def weigh_view_ray_layers(lib, view, rays, hits, lods=None, stream=None):
    """RT64_WeighViewRayLayers: (N, 8) float32 rays, the (L, N, 8) float32 hits trace_view_ray_layers returned for them (1 <= L <= 16, layer-major) and, optionally,
    (N,) float32 lods -> (weights (L, N) float32, coverage (N, 4)): the share of the picture a frame's resolve gives each layer, and per ray transmittance, refraction
    (float32) and shaded, flags (uint32 bits: read the array through `.view(uint32)`) -- rule T7.  NumPy arrays take the host path; torch CUDA tensors the device
    path, enqueued on `stream` like trace_rays."""
    on_device = _is_torch(rays)
    if on_device:
        import torch
        if not _is_torch(hits) or hits.dim() != 3 or hits.shape[2] != 8 or hits.dtype != torch.float32 or not hits.is_cuda:
            raise ValueError("hits: an (L, N, 8) float32 CUDA tensor")
        hits = hits.contiguous()
        address = hits.data_ptr()
    else:
        import numpy as np
        hits = np.ascontiguousarray(hits, dtype=np.float32)
        if hits.ndim != 3 or hits.shape[2] != 8:
            raise ValueError("hits: an (L, N, 8) float32 array")
        address = hits.ctypes.data
    layers = _layer_count(hits.shape[0])
    if hits.shape[1] != rays.shape[0]:
        raise ValueError("one list of hits per ray")
    if on_device and stream is not None and stream != torch.cuda.current_stream(hits.device):
        hits.record_stream(stream)
    weights, coverage = _query(lib, view, "WeighViewRayLayers", "WeighViewRayLayersDevice",
                               [("in", rays), ("value", address), ("lods", lods), ("value", layers), ("out", (layers, 1)), ("out", 4)], None, stream)
    return weights.reshape(layers, -1), coverage


def trace_view_ray_layers(lib, view, rays, max_layers, lods=None, flags=0, weights=False, stream=None):
    """RT64_TraceViewRayLayers: (N, 8) float32 rays and, optionally, (N,) float32 lods -> (hits (L, N, 8) float32, layers (N, 4) uint32) with L = max_layers (1..16):
    per ray the sorted hit list a frame keeps -- key t - depthBias, cut at its first opaque entry, rules T1-T6 -- layer-major, the entries behind a list's end the miss
    record; `layers` holds count, flags, nodesVisited, trianglesTested.  With `weights` the result is (hits, layers, weights (L, N), coverage (N, 4)) as
    weigh_view_ray_layers returns them (T8).  `flags`: RAY_FLAG_CULL_BACK_FACING only.  NumPy arrays take the host path (one staging round trip, weights included); torch
    CUDA tensors the device path, enqueued on `stream` like trace_rays."""
    L = _layer_count(max_layers)
    if _is_torch(rays):
        hits, layers = _query(lib, view, "TraceViewRayLayers", "TraceViewRayLayersDevice", [("in", rays), ("lods", lods), ("value", L), ("out", (L, 8)), ("out", 4)], flags, stream)
        if not weights:
            return hits, _as_uint32(layers)
        return (hits, _as_uint32(layers)) + tuple(weigh_view_ray_layers(lib, view, rays, hits, lods, stream))
    outs = _query(lib, view, "TraceViewRayLayers", None,
                  [("in", rays), ("lods", lods), ("value", L), ("out", (L, 8)), ("out", 4), ("out", (L, 1) if weights else None), ("out", 4 if weights else None)], flags)
    if not weights:
        return outs[0], _as_uint32(outs[1])
    return outs[0], _as_uint32(outs[1]), outs[2].reshape(L, -1), outs[3]


def sky_view_rays(lib, view, rays, stream=None):
    """RT64_SkyViewRays: (N, 8) float32 rays -> (N, 8) float32 RT64_RAY_SKYs: color rgb, alpha, uv, then flags and reserved as uint32 bits (read them through
    `.view(uint32)`): what a mirror, glass or GI ray of the view's last frame sees when it misses everything -- the sky texture along the direction as given, over
    the frame's raster background (rule W1).  NumPy arrays take the host path; torch CUDA tensors the device path, enqueued on `stream` like trace_rays."""
    return _query(lib, view, "SkyViewRays", "SkyViewRaysDevice", [("in", rays), ("out", 8)], None, stream)


def sky_view_pixels(lib, view, pixels=None, count=None, stream=None):
    """RT64_SkyViewPixels: `pixels` as camera_rays takes them -- an (N, 2) uint32 array of (x, y), or None with `count`: the frame's first `count` pixels row by row --
    -> (N, 8) float32 RT64_RAY_SKYs as sky_view_rays returns them: what a camera ray of the view's last frame shows when it misses everything, the sky plane at
    screenUV = (p + jitter) / size over the raster background (rule W2).  A NumPy array takes the host path; a torch CUDA tensor the device path, enqueued on `stream`."""
    return _pixel_query(lib, view, "SkyViewPixels", "SkyViewPixelsDevice", pixels, count, [8], None, stream)


def resolve_view_ray_radiance(lib, view, rays, hits, lods=None, flags=0, stream=None):
    """RT64_ComposeViewRayRadiance: (N, 8) float32 rays, the (L, N, 8) float32 hits trace_view_ray_layers returned for them (1 <= L <= 16, layer-major) and, optionally,
    (N,) float32 lods -> (N, 16) float32 RT64_RAY_RADIANCEs: radiance rgb, flags, surface rgb, transmittance, transparent rgb, litLayer, light rgb, layers (flags,
    litLayer, layers as uint32 / int32 bits: read them through `.view(int32)`): the colour the ray brings back in the secondary-ray resolve of the view's last frame
    (rules W3-W7).  `flags`: RAY_FLAG_CULL_BACK_FACING, RADIANCE_FLAG_UNSHADOWED, RADIANCE_FLAG_FOG_FROM_CAMERA.  NumPy arrays take the host path; torch CUDA tensors
    the device path, enqueued on `stream` like trace_rays."""
    on_device = _is_torch(rays)
    if on_device:
        import torch
        if not _is_torch(hits) or hits.dim() != 3 or hits.shape[2] != 8 or hits.dtype != torch.float32 or not hits.is_cuda:
            raise ValueError("hits: an (L, N, 8) float32 CUDA tensor")
        hits = hits.contiguous()
        address = hits.data_ptr()
    else:
        import numpy as np
        hits = np.ascontiguousarray(hits, dtype=np.float32)
        if hits.ndim != 3 or hits.shape[2] != 8:
            raise ValueError("hits: an (L, N, 8) float32 array")
        address = hits.ctypes.data
    layers = _layer_count(hits.shape[0])
    if hits.shape[1] != rays.shape[0]:
        raise ValueError("one list of hits per ray")
    if on_device and stream is not None and stream != torch.cuda.current_stream(hits.device):
        hits.record_stream(stream)
    return _query(lib, view, "ComposeViewRayRadiance", "ComposeViewRayRadianceDevice",
                  [("in", rays), ("value", address), ("lods", lods), ("value", layers), ("out", 16)], flags, stream)


def trace_view_ray_radiance(lib, view, rays, max_layers=RAY_LAYERS_MAX, lods=None, flags=0, hits=True, layers=True):
    """RT64_TraceViewRayRadiance on an (N, 8) float32 NumPy array of rays (and optional (N,) float32 lods): the walk of trace_view_ray_layers and the records of
    resolve_view_ray_radiance in one staging round trip -> (hits (L, N, 8), layers (N, 4) uint32, radiance (N, 16)) with L = max_layers; `hits`, `layers` = False
    passes NULL for that output and leaves it out of the result (rule W8)."""
    L = _layer_count(max_layers)
    outs = _query(lib, view, "TraceViewRayRadiance", None,
                  [("in", rays), ("lods", lods), ("value", L), ("out", (L, 8) if hits else None), ("out", 4 if layers else None), ("out", 16)], flags)
    if not hits and not layers:
        return outs
    outs = list(outs)
    if layers:
        outs[1 if hits else 0] = _as_uint32(outs[1 if hits else 0])
    return tuple(outs)


GI_POINT_DTYPE = [("position", "<f4", (3,)), ("flags", "<u4"), ("normal", "<f4", (3,)), ("instance", "<i4")]          # numpy dtypes of the four structs of rt64_indirect.h
GI_SAMPLING_DTYPE = [("giSamples", "<i4"), ("giBounces", "<i4"), ("diSamples", "<i4"), ("flags", "<u4")]
GI_SAMPLE_DTYPE = [("radiance", "<f4", (3,)), ("remaining", "<f4"), ("position", "<f4", (3,)), ("flags", "<u4"), ("normal", "<f4", (3,)), ("instance", "<i4"),
                   ("layers", "<u4"), ("reserved", "<u4"), ("nodesVisited", "<u4"), ("trianglesTested", "<u4")]
POINT_INDIRECT_DTYPE = [("indirect", "<f4", (3,)), ("samples", "<f4"), ("moments", "<f4", (2,)), ("flags", "<u4"), ("instance", "<i4"),
                        ("rays", "<u4"), ("nodesVisited", "<u4"), ("trianglesTested", "<u4"), ("reserved", "<u4")]


def _gi_sampling(gi_samples, gi_bounces, di_samples):
    """RT64_GI_SAMPLING of the three overrides (-1: the last frame's value) -> (address or None for NULL, the struct to keep alive)."""
    if gi_samples == -1 and gi_bounces == -1 and di_samples == -1:
        return None, None
    s = GI_SAMPLING(int(gi_samples), int(gi_bounces), int(di_samples), 0)
    return C.addressof(s), s


def _gi_points(points):
    """The points argument of the indirect-light wrappers: an (N, 8) float32 array (position xyz, flags, normal xyz, instance; the two integers as bits), or a structured
    array of GI_POINT_DTYPE, which is viewed as one."""
    if not _is_torch(points):
        import numpy as np
        points = np.asarray(points)
        if points.dtype.names is not None:
            points = np.ascontiguousarray(points, dtype=np.dtype(GI_POINT_DTYPE)).view(np.float32).reshape(-1, 8)
    return points


def gi_rays(lib, view, points, slot, keys=None, gi_samples=-1, second_bounce=False, stream=None):
    """RT64_GenerateViewPointGIRays: (N, 8) float32 RT64_GI_POINTs (or a structured array of GI_POINT_DTYPE) and, optionally, (N, 4) uint32 keys (None: point i is keyed
    as pixel i of the last frame) -> (N, 8) float32 RT64_RAYs: the bounce ray of sample `slot` (giSamples .. 1) of every point as the frame's GI pass sends it, or with
    `second_bounce` on the second bounce's noise slice (rule Y4).  `gi_samples` (1 .. 64) overrides the frame's value; -1 keeps it.  NumPy arrays take the host path; torch
    CUDA tensors the device path, enqueued on `stream` like trace_rays."""
    points = _gi_points(points)
    k, keep_k = _sample_keys(points, keys, stream)
    p, keep_p = _gi_sampling(gi_samples, -1, -1)
    return _query(lib, view, "GenerateViewPointGIRays", "GenerateViewPointGIRaysDevice",
                  [("in", points), ("value", k), ("value", p), ("value", int(slot)), ("value", GI_RAYS_SECOND_BOUNCE if second_bounce else 0), ("out", 8)], None, stream)


def shade_gi_rays(lib, view, rays, hits, keys=None, incoming=None, di_samples=-1, stream=None):
    """RT64_ComposeViewGIRays: (N, 8) float32 bounce rays, the (L, N, 8) float32 hits trace_view_ray_layers returned for them (RAY_FLAG_CULL_BACK_FACING, no lods), optional
    (N, 4) uint32 keys and optional (N, 3) float32 `incoming` (None: the frame's ambient term) -> (N, 16) float32 RT64_GI_SAMPLEs: radiance rgb, remaining, position xyz,
    flags, normal xyz, instance, layers, reserved, nodesVisited, trianglesTested (view the array through GI_SAMPLE_DTYPE): what one GI ray of the frame brings back (rules
    Y5-Y7).  `di_samples` (0 .. 64) overrides the frame's value.  NumPy arrays take the host path; torch CUDA tensors the device path, enqueued on `stream`."""
    on_device = _is_torch(rays)
    n = rays.shape[0] if hasattr(rays, "shape") and len(rays.shape) else -1
    if on_device:
        import torch
        if not _is_torch(hits) or hits.dim() != 3 or hits.shape[2] != 8 or hits.dtype != torch.float32 or not hits.is_cuda:
            raise ValueError("hits: an (L, N, 8) float32 CUDA tensor")
        if incoming is not None and (not _is_torch(incoming) or tuple(incoming.shape) != (n, 3) or incoming.dtype != torch.float32 or not incoming.is_cuda):
            raise ValueError("incoming: an (N, 3) float32 CUDA tensor")
        hits = hits.contiguous(); incoming = incoming.contiguous() if incoming is not None else None
        address = lambda a: a.data_ptr()
    else:
        import numpy as np
        hits = np.ascontiguousarray(hits, dtype=np.float32)
        if hits.ndim != 3 or hits.shape[2] != 8:
            raise ValueError("hits: an (L, N, 8) float32 array")
        if incoming is not None:
            incoming = np.ascontiguousarray(incoming, dtype=np.float32)
            if incoming.shape != (n, 3):
                raise ValueError("incoming: an (N, 3) float32 array")
        address = lambda a: a.ctypes.data
    layers = _layer_count(hits.shape[0])
    if hits.shape[1] != n:
        raise ValueError("one list of hits per ray")
    if on_device and stream is not None and stream != torch.cuda.current_stream(hits.device):
        hits.record_stream(stream)
        if incoming is not None:
            incoming.record_stream(stream)
    k, keep_k = _sample_keys(rays, keys, stream)
    p, keep_p = _gi_sampling(-1, -1, di_samples)
    return _query(lib, view, "ComposeViewGIRays", "ComposeViewGIRaysDevice",
                  [("in", rays), ("value", address(hits)), ("value", layers), ("value", k), ("value", address(incoming) if incoming is not None else None), ("value", p), ("out", 16)], None, stream)


def sample_indirect(lib, view, points, keys=None, gi_samples=-1, gi_bounces=-1, di_samples=-1, samples=False, stream=None):
    """RT64_TraceViewPointsIndirect: (N, 8) float32 RT64_GI_POINTs (or a structured array of GI_POINT_DTYPE) and, optionally, (N, 4) uint32 keys -> (N, 12) float32
    RT64_POINT_INDIRECTs: indirect rgb, samples, moments, flags, instance, rays, nodesVisited, trianglesTested, reserved (view the array through POINT_INDIRECT_DTYPE): the
    indirect light of each point as the frame's GI pass computes it for the pixel of the key, without history (rule Y8).  `gi_samples` (0 .. 64), `gi_bounces` (1, 2) and
    `di_samples` (0 .. 64) override the frame's values; -1 keeps them.  With `samples` -- it needs `gi_samples` given -- the result is (records, samples (S, N, 16)): the
    first bounce's RT64_GI_SAMPLEs, sample slot S - k in block k.  NumPy arrays take the host path; torch CUDA tensors the device path, enqueued on `stream`."""
    points = _gi_points(points)
    if samples and gi_samples < 0:
        raise ValueError("samples: give gi_samples, the array is sized by it")
    k, keep_k = _sample_keys(points, keys, stream)
    p, keep_p = _gi_sampling(gi_samples, gi_bounces, di_samples)
    want = samples and gi_samples > 0
    outs = _query(lib, view, "TraceViewPointsIndirect", "TraceViewPointsIndirectDevice",
                  [("in", points), ("value", k), ("value", p), ("out", (int(gi_samples), 16) if want else None), ("out", 12)], None, stream)
    if not samples:
        return outs
    if want:
        return outs[1], outs[0]
    return outs, outs[:0].reshape(0, outs.shape[0], 16) if not _is_torch(outs) else outs.new_empty((0, outs.shape[0], 16))


def trace_indirect(lib, view, rays, lods=None, keys=None, gi_samples=-1, gi_bounces=-1, di_samples=-1, flags=0):
    """RT64_TraceViewRayIndirect on an (N, 8) float32 NumPy array of rays (optional (N,) float32 lods and (N, 4) uint32 keys): the walk of trace_rays_alpha, the point of
    each hit and the records of sample_indirect in one staging round trip per chunk -> (hits (N, 8), records (N, 12)); a miss gives a zero record with instance -1 (rule
    Y10).  `flags`: RAY_FLAG_CULL_BACK_FACING only."""
    k, keep_k = _sample_keys(rays, keys, None)
    p, keep_p = _gi_sampling(gi_samples, gi_bounces, di_samples)
    return _query(lib, view, "TraceViewRayIndirect", None, [("in", rays), ("out", 8), ("lods", lods), ("value", k), ("value", p), ("out", 12)], flags)
