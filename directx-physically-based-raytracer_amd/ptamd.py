"""ctypes binding of libptamd.so (include/ptamd.h) + the Python mirror of the reference's operators.

Mirror of the reference interface for this path (same names, argument meaning, error behaviour):
  Scene.CreateAccelerationStructures / GetTopLevelAccelerationStructure   Source/Scene.ixx:282-380
  GBufferGeneration{GPUBuffers, Textures, Render(constants)}              Source/GBufferGeneration.ixx:27-122
  Raytracing{GPUBuffers, Textures, SetConstants, Render}                  Source/Raytracing.ixx:29-250
PyTorch is used only as plumbing: device memory (uint8 tensors), streams, torch.distributed.
There is NO CPU fallback: if libptamd.so is missing or no GPU is visible this module raises.
"""
import ctypes as C
import os

import numpy as np

from . import layouts as L

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libptamd.so")
_LIB = None

EXPORTS = [
    "pt_abi_version", "pt_create", "pt_destroy", "pt_last_error", "pt_set_stream", "pt_sync", "pt_set_frames_in_flight", "pt_set_round_chains",
    "pt_heap_resize", "pt_heap_set_buffer", "pt_heap_set_texture", "pt_build_bottom_level", "pt_update_bottom_level", "pt_release_bottom_level", "pt_skin_mesh",
    "pt_build_top_level", "pt_build_top_level_posed", "pt_get_accel_stats", "pt_share_scene", "pt_set_camera", "pt_set_scene_data", "pt_set_object_data", "pt_invalidate_object_data",
    "pt_set_instance_data", "pt_set_sharding", "pt_local_rows", "pt_deinterleave_bands", "pt_gbuffer_render",
    "pt_comm_get_unique_id", "pt_comm_init", "pt_comm_adopt", "pt_comm_destroy", "pt_gather_bands", "pt_gather_plan",
    "pt_raytrace_set_constants", "pt_raytrace_render", "pt_trace_visibility", "pt_bsdf_evaluate", "pt_bsdf_sample", "pt_reset_counters", "pt_get_counters",
    "pt_di_set_constants", "pt_di_render", "pt_di_light_count", "pt_di_download_lights",
    "pt_di_set_resampling", "pt_di_render_with_history", "pt_di_reset_history", "pt_di_download_reservoirs",
    "pt_di_set_light_sampling", "pt_di_download_presampled", "pt_di_set_visibility", "pt_di_set_pairwise",
    "pt_di_set_regir_layout", "pt_di_regir_onion_table", "pt_di_set_brdf_sampling", "pt_di_download_brdf_candidates",
    "pt_di_pdf_texture_size", "pt_di_set_pdf_mipmap", "pt_di_download_pdf_texture", "pt_mipmap_generate",
    "pt_post_set_constants", "pt_post_render", "pt_post_download_bloom",
    "pt_nrd_composition_process", "pt_nrd_composition_pixels_per_lane", "pt_nrd_reblur_hit_distance_defaults",
    "pt_denoiser_set_constants", "pt_denoiser_process", "pt_denoiser_reset_history", "pt_denoiser_download_history",
    "pt_upscaler_set_constants", "pt_upscaler_process", "pt_upscaler_reset_history", "pt_upscaler_download_history",
    "pt_upscaler_render_size", "pt_upscaler_jitter",
    "pt_reconstruction_set_constants", "pt_reconstruction_process", "pt_reconstruction_reset_history", "pt_reconstruction_download_history",
    "pt_frame_generation_set_constants", "pt_frame_generation_process", "pt_frame_generation_reset_history", "pt_frame_generation_download_field",
    "pt_sharpen_set_constants", "pt_sharpen_process",
    "pt_anim_create_rig", "pt_anim_release_rig", "pt_anim_create_object", "pt_anim_release_object", "pt_anim_evaluate",
    "pt_anim_skeletal_transforms", "pt_anim_download_globals", "pt_anim_download_skeletal", "pt_anim_debug_slerp",
    "pt_sharc_configure", "pt_sharc_set_constants", "pt_raytrace_render_sharc", "pt_sharc_reset", "pt_sharc_download",
    "pt_sharc_debug_keys", "pt_sharc_debug_query", "pt_sharc_download_update_paths", "pt_sharc_download_update_scatter",
    "pt_set_debug_flags", "pt_debug_read_mismatch", "pt_debug_download_blob", "pt_debug_trace_ray", "pt_debug_trace_closest", "pt_enable_kernel_timing", "pt_get_kernel_timing", "pt_get_round_timing",
]


class PtError(RuntimeError):
    """reference: std::system_error from ThrowIfFailed (Source/ErrorHelpers.ixx:16-32)."""


class PtInvalidArgument(ValueError):
    """reference: Throw<std::invalid_argument> (Source/RaytracingHelpers.ixx:83-88)."""


class GeometryDesc(C.Structure):
    _fields_ = [("VertexBuffer", C.c_void_p), ("VertexCount", C.c_uint32), ("VertexStride", C.c_uint32),
                ("IndexBuffer", C.c_void_p), ("IndexCount", C.c_uint32), ("IndexStride", C.c_uint32),
                ("Flags", C.c_uint32), ("_pad", C.c_uint32)]


class InstanceDesc(C.Structure):
    _fields_ = [("Transform", C.c_float * 12), ("InstanceID", C.c_uint32), ("InstanceMask", C.c_uint32),
                ("AccelerationStructure", C.c_uint64)]


TEXTURE_NAMES = L.GBUFFER_ORDER + ["RadianceF32", "Diffuse", "Specular", "SpecularHitDistance"]


class Textures(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in TEXTURE_NAMES]


class PreviousTextures(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in L.DI_PREVIOUS_TEXTURES]


class PostTextures(C.Structure):
    _fields_ = [("Radiance", C.c_void_p), ("Color", C.c_void_p), ("BackBuffer", C.c_void_p), ("Display8", C.c_void_p)]


class NRDCompositionTextures(C.Structure):   # PtNRDCompositionTextures: nine pointers, NRDComposition::Textures' member order
    _fields_ = [(n, C.c_void_p) for n in L.NRD_COMPOSITION_TEXTURES]


class DenoiserTextures(C.Structure):         # PtDenoiserTextures: eight pointers
    _fields_ = [(n, C.c_void_p) for n in L.DENOISER_TEXTURES]


class UpscalerTextures(C.Structure):         # PtUpscalerTextures: four pointers
    _fields_ = [(n, C.c_void_p) for n in L.UPSCALER_TEXTURES]


class ReconstructionTextures(C.Structure):   # PtReconstructionTextures: eight pointers
    _fields_ = [(n, C.c_void_p) for n in L.RECONSTRUCTION_TEXTURES]


class FrameGenerationTextures(C.Structure): # PtFrameGenerationTextures: five pointers
    _fields_ = [(n, C.c_void_p) for n in L.FRAME_GENERATION_TEXTURES]


class SharpenTextures(C.Structure):         # PtSharpenTextures: two pointers
    _fields_ = [(n, C.c_void_p) for n in L.SHARPEN_TEXTURES]


class Sharding(C.Structure):
    _fields_ = [("RankIndex", C.c_uint32), ("RankCount", C.c_uint32), ("BandHeight", C.c_uint32), ("_pad", C.c_uint32)]


class BandMessage(C.Structure):
    _fields_ = [("Peer", C.c_uint32), ("IsSend", C.c_uint32), ("Band", C.c_uint32), ("_pad", C.c_uint32),
                ("LocalOffset", C.c_uint64), ("FullOffset", C.c_uint64), ("Bytes", C.c_uint64)]


class Counters(C.Structure):
    _fields_ = [("PrimaryRays", C.c_uint64), ("SecondaryRays", C.c_uint64), ("NodesVisited", C.c_uint64),
                ("TrianglesTested", C.c_uint64), ("WavefrontIterations", C.c_uint64), ("BvhMismatches", C.c_uint64),
                ("StackOverflows", C.c_uint64), ("MaxNodesPerRay", C.c_uint64)]


class BlobLayout(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("InstanceOffset16", "NodeOffset16", "TriangleOffset16", "LeafInstanceOffset16",
                                          "InstanceCount", "NodeCount", "TriangleCount", "Bytes")]


class AccelStats(C.Structure):
    _fields_ = [("InstanceCount", C.c_uint32), ("BottomLevelCount", C.c_uint32), ("TriangleCount", C.c_uint64),
                ("NodeBytes", C.c_uint64), ("TriangleBytes", C.c_uint64), ("NodeSizeBytes", C.c_uint32),
                ("TriangleSizeBytes", C.c_uint32), ("MaxBottomLevelDepth", C.c_uint32), ("TopLevelDepth", C.c_uint32),
                ("BlobBytes", C.c_uint64), ("SharedScene", C.c_uint32), ("NormalRecords", C.c_uint32),
                ("OwnedBottomLevelBytes", C.c_uint64), ("RoundObjectsInLds", C.c_uint32), ("RoundRecordsInLds", C.c_uint32)]


_BSDF_MATERIAL = [("BaseColor", C.c_float * 3), ("Metallic", C.c_float), ("Roughness", C.c_float), ("IOR", C.c_float),
                  ("Transmission", C.c_float), ("IsFrontFace", C.c_float),
                  ("GeometricNormal", C.c_float * 3), ("ShadingNormal", C.c_float * 3), ("V", C.c_float * 3)]


class BsdfQuery(C.Structure):
    _fields_ = _BSDF_MATERIAL + [("L", C.c_float * 3)]


class BsdfResult(C.Structure):
    _fields_ = [("Diffuse", C.c_float * 3), ("Specular", C.c_float * 3), ("PDF", C.c_float), ("_pad", C.c_float)]


class BsdfSampleQuery(C.Structure):
    _fields_ = _BSDF_MATERIAL + [("Random", C.c_float * 4), ("ExtFlags", C.c_uint32), ("_pad", C.c_uint32 * 2)]


class BsdfSampleResult(C.Structure):
    _fields_ = [("L", C.c_float * 3), ("PDF", C.c_float), ("F", C.c_float * 3), ("Weights", C.c_float * 3),
                ("Lobe", C.c_uint32), ("Ok", C.c_uint32)]


class AnimState(C.Structure):               # struct PtAnimState, 24 B
    _fields_ = [("Object", C.c_uint64), ("Clip", C.c_uint32), ("_pad", C.c_uint32), ("Time", C.c_double)]


CLOSEST_HIT = np.dtype([("T", "<f4"), ("U", "<f4"), ("V", "<f4"), ("Instance", "<u4"), ("Geometry", "<u4"), ("Primitive", "<u4"),
                        ("Slot", "<u4"), ("_pad", "<u4")])          # PtClosestHit, 32 B


def load_library():
    """Load libptamd.so; fail loudly when the HIP extension has not been built."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise PtError(f"{LIB_PATH} is missing: run __graft_entry__.build() (make -C .../csrc). "
                          "The path tracer has no CPU fallback.")
        # torch bundles its own libamdhip64.so.7; import it first so libptamd.so binds to the SAME HIP
        # runtime (two runtimes in one process cannot both open the device, and tensors would not be shared)
        import torch  # noqa: F401
        lib = C.CDLL(LIB_PATH)
        lib.pt_last_error.restype = C.c_char_p
        lib.pt_last_error.argtypes = [C.c_void_p]
        lib.pt_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
        lib.pt_destroy.argtypes = [C.c_void_p]; lib.pt_destroy.restype = None
        lib.pt_set_stream.argtypes = [C.c_void_p, C.c_void_p]
        lib.pt_sync.argtypes = [C.c_void_p]
        lib.pt_set_frames_in_flight.argtypes = [C.c_void_p, C.c_uint32]
        lib.pt_set_round_chains.argtypes = [C.c_void_p, C.c_uint32]
        lib.pt_heap_resize.argtypes = [C.c_void_p, C.c_uint32]
        lib.pt_heap_set_buffer.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint32]
        lib.pt_heap_set_texture.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]
        lib.pt_build_bottom_level.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]
        lib.pt_release_bottom_level.argtypes = [C.c_void_p, C.c_uint64]
        lib.pt_update_bottom_level.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_uint32]
        lib.pt_skin_mesh.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
        lib.pt_build_top_level.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
        lib.pt_build_top_level_posed.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        lib.pt_anim_create_rig.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_uint32, C.POINTER(C.c_uint64)]
        lib.pt_anim_release_rig.argtypes = [C.c_void_p, C.c_uint64]
        lib.pt_anim_create_object.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]
        lib.pt_anim_release_object.argtypes = [C.c_void_p, C.c_uint64]
        lib.pt_anim_evaluate.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        lib.pt_anim_skeletal_transforms.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_uint32)]
        lib.pt_anim_download_globals.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
        lib.pt_anim_download_skeletal.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
        lib.pt_anim_debug_slerp.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        lib.pt_get_accel_stats.argtypes = [C.c_void_p, C.c_void_p]
        lib.pt_share_scene.argtypes = [C.c_void_p, C.c_void_p]
        for f in (lib.pt_set_camera, lib.pt_set_scene_data, lib.pt_set_sharding, lib.pt_raytrace_set_constants,
                  lib.pt_raytrace_render, lib.pt_get_counters):
            f.argtypes = [C.c_void_p, C.c_void_p]
        lib.pt_set_object_data.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        lib.pt_set_instance_data.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        lib.pt_invalidate_object_data.argtypes = [C.c_void_p]
        lib.pt_local_rows.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
        lib.pt_deinterleave_bands.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                              C.c_uint32, C.c_uint32, C.c_uint32]
        lib.pt_comm_get_unique_id.argtypes = [C.c_void_p]
        lib.pt_comm_init.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
        lib.pt_comm_adopt.argtypes = [C.c_void_p, C.c_void_p]
        lib.pt_comm_destroy.argtypes = [C.c_void_p]
        lib.pt_gather_bands.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]
        lib.pt_gather_plan.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
        lib.pt_gbuffer_render.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        lib.pt_trace_visibility.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        lib.pt_bsdf_evaluate.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        lib.pt_bsdf_sample.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        lib.pt_reset_counters.argtypes = [C.c_void_p]
        lib.pt_di_set_constants.argtypes = [C.c_void_p, C.c_void_p]
        lib.pt_di_render.argtypes = [C.c_void_p, C.c_void_p]
        lib.pt_di_light_count.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        lib.pt_di_download_lights.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
        lib.pt_di_set_resampling.argtypes = [C.c_void_p, C.c_void_p]
        lib.pt_di_render_with_history.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        lib.pt_di_reset_history.argtypes = [C.c_void_p]
        lib.pt_di_download_reservoirs.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
        lib.pt_di_set_light_sampling.argtypes = [C.c_void_p, C.c_void_p]
        lib.pt_di_set_visibility.argtypes = [C.c_void_p, C.c_void_p]
        lib.pt_di_set_pairwise.argtypes = [C.c_void_p, C.c_void_p]
        lib.pt_di_set_regir_layout.argtypes = [C.c_void_p, C.c_void_p]
        lib.pt_di_regir_onion_table.argtypes = [C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
        lib.pt_di_download_presampled.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
        lib.pt_di_set_brdf_sampling.argtypes = [C.c_void_p, C.c_uint32, C.c_float]
        lib.pt_di_download_brdf_candidates.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
        lib.pt_di_pdf_texture_size.argtypes = [C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        lib.pt_di_set_pdf_mipmap.argtypes = [C.c_void_p, C.c_uint32]
        lib.pt_di_download_pdf_texture.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        lib.pt_mipmap_generate.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32]
        lib.pt_post_set_constants.argtypes = [C.c_void_p, C.c_void_p]
        lib.pt_post_render.argtypes = [C.c_void_p, C.c_void_p]
        lib.pt_post_download_bloom.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        lib.pt_nrd_composition_process.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        lib.pt_nrd_composition_pixels_per_lane.argtypes = [C.c_void_p, C.c_void_p]
        lib.pt_nrd_reblur_hit_distance_defaults.argtypes = [C.c_void_p]; lib.pt_nrd_reblur_hit_distance_defaults.restype = None
        lib.pt_denoiser_set_constants.argtypes = [C.c_void_p, C.c_void_p]
        lib.pt_denoiser_process.argtypes = [C.c_void_p, C.c_void_p]
        lib.pt_denoiser_reset_history.argtypes = [C.c_void_p]
        lib.pt_denoiser_download_history.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        lib.pt_upscaler_set_constants.argtypes = [C.c_void_p, C.c_void_p]
        lib.pt_upscaler_process.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_float)]
        lib.pt_upscaler_reset_history.argtypes = [C.c_void_p]
        lib.pt_upscaler_download_history.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        lib.pt_upscaler_render_size.argtypes = [C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        lib.pt_upscaler_jitter.argtypes = [C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_float)]
        lib.pt_reconstruction_set_constants.argtypes = [C.c_void_p, C.c_void_p]
        lib.pt_reconstruction_process.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_float)]
        lib.pt_reconstruction_reset_history.argtypes = [C.c_void_p]
        lib.pt_reconstruction_download_history.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                                           C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        lib.pt_frame_generation_set_constants.argtypes = [C.c_void_p, C.c_void_p]
        lib.pt_frame_generation_process.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_uint32)]
        lib.pt_frame_generation_reset_history.argtypes = [C.c_void_p]
        lib.pt_frame_generation_download_field.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                                           C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        lib.pt_sharpen_set_constants.argtypes = [C.c_void_p, C.c_void_p]
        lib.pt_sharpen_process.argtypes = [C.c_void_p, C.c_void_p]
        lib.pt_sharc_configure.argtypes = [C.c_void_p, C.c_uint32]
        lib.pt_sharc_set_constants.argtypes = [C.c_void_p, C.c_void_p]
        lib.pt_raytrace_render_sharc.argtypes = [C.c_void_p, C.c_void_p]
        lib.pt_sharc_reset.argtypes = [C.c_void_p]
        lib.pt_sharc_download.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
        lib.pt_sharc_debug_keys.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.pt_sharc_debug_query.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        lib.pt_sharc_download_update_paths.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        lib.pt_sharc_download_update_scatter.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        lib.pt_set_debug_flags.argtypes = [C.c_void_p, C.c_uint32]
        lib.pt_debug_read_mismatch.argtypes = [C.c_void_p, C.c_void_p]
        lib.pt_debug_download_blob.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
        lib.pt_debug_trace_ray.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
        lib.pt_debug_trace_closest.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        lib.pt_enable_kernel_timing.argtypes = [C.c_void_p, C.c_int]
        lib.pt_get_round_timing.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_uint32)]
        lib.pt_get_kernel_timing.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                             C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        _LIB = lib
    return _LIB


def local_rows(height, rank=0, world=1, band=16):
    s = Sharding(rank, world, band, 0)
    out = C.c_uint32(0)
    if load_library().pt_local_rows(C.byref(s), height, C.byref(out)) != 0:
        raise PtInvalidArgument("invalid sharding")
    return out.value


def gather_plan(height, row_bytes, rank, world, band=16, root=0):
    """pt_gather_plan: the (peer, is_send, band, local_offset, full_offset, bytes) messages rank `rank` issues in a gather. No GPU."""
    lib = load_library()
    s = Sharding(rank, world, band, 0)
    n = C.c_uint32(0)
    if lib.pt_gather_plan(C.byref(s), height, row_bytes, root, None, 0, C.byref(n)) != 0:
        raise PtInvalidArgument("invalid sharding / root")
    msgs = (BandMessage * max(1, n.value))()
    if lib.pt_gather_plan(C.byref(s), height, row_bytes, root, msgs, n.value, C.byref(n)) != 0:
        raise PtInvalidArgument("invalid sharding / root")
    return [(m.Peer, m.IsSend, m.Band, m.LocalOffset, m.FullOffset, m.Bytes) for m in msgs[:n.value]]


class DeviceContext:
    """One per GPU (reference: DeviceContext/CommandList pair, one D3D12 device)."""

    def __init__(self, device_ordinal=0, stream=None):
        self.lib = load_library()
        h = C.c_void_p()
        st = self.lib.pt_create(device_ordinal, C.byref(h))
        if st != 0:
            raise PtError(f"pt_create failed ({st}): {self.lib.pt_last_error(None).decode()}")
        self.handle = h
        self.device_ordinal = device_ordinal
        if stream is not None:
            self.check(self.lib.pt_set_stream(self.handle, C.c_void_p(stream)))

    def check(self, status):
        if status == 0:
            return
        msg = self.lib.pt_last_error(self.handle).decode()
        if status == -1:
            raise PtInvalidArgument(msg)
        raise PtError(f"status {status}: {msg}")

    def sync(self):
        self.check(self.lib.pt_sync(self.handle))

    def set_frames_in_flight(self, n):
        self.check(self.lib.pt_set_frames_in_flight(self.handle, n))

    def set_round_chains(self, n):
        """0 = the library's choice; n independent chains of launches per frame (pt_set_round_chains)."""
        self.check(self.lib.pt_set_round_chains(self.handle, n))

    def close(self):
        if getattr(self, "handle", None):
            self.lib.pt_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # measurement ---------------------------------------------------------------------------
    def reset_counters(self):
        self.check(self.lib.pt_reset_counters(self.handle))

    def counters(self):
        c = Counters()
        self.check(self.lib.pt_get_counters(self.handle, C.byref(c)))
        return c

    def set_debug_flags(self, flags):
        self.check(self.lib.pt_set_debug_flags(self.handle, flags))
        self.debug_flags = flags

    def invalidate_object_data(self):
        """VertexDesc / MeshDescriptors of the bound ObjectData were rewritten in place: resolve and check them again at the next render."""
        self.check(self.lib.pt_invalidate_object_data(self.handle))

    def enable_kernel_timing(self, on=True):
        self.check(self.lib.pt_enable_kernel_timing(self.handle, 1 if on else 0))

    def kernel_timing(self):
        e, s, ne, ns = C.c_float(), C.c_float(), C.c_uint32(), C.c_uint32()
        self.check(self.lib.pt_get_kernel_timing(self.handle, C.byref(e), C.byref(s), C.byref(ne), C.byref(ns)))
        r, nr = C.c_float(), C.c_uint32()
        self.check(self.lib.pt_get_round_timing(self.handle, C.byref(r), C.byref(nr)))
        return {"extend_ms": e.value, "shade_ms": s.value, "extend_launches": ne.value, "shade_launches": ns.value,
                "round_ms": r.value, "round_launches": nr.value}

    def download_blob(self):
        """(layout, bytes) of the traversal copy of the scene -- for the structural checks in tests/."""
        lay = BlobLayout()
        self.check(self.lib.pt_debug_download_blob(self.handle, None, 0, C.byref(lay)))
        buf = np.zeros(lay.Bytes, np.uint8)
        self.check(self.lib.pt_debug_download_blob(self.handle, C.c_void_p(buf.ctypes.data), buf.nbytes, C.byref(lay)))
        return lay, buf

    def trace_closest(self, rays, brute_force=False):
        """pt_debug_trace_closest over host rays [n, 8] float32 (origin, tmin, direction, tmax): CLOSEST_HIT records. brute_force: with
        PT_DEBUG_BRUTE_FORCE set for the call (every triangle of every instance, no box test); the flags set through set_debug_flags are
        back in place afterwards."""
        torch = _torch()
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        dr = torch.from_numpy(rays).to(torch.device("cuda", self.device_ordinal))
        dh = torch.zeros(max(1, len(rays)) * 32, dtype=torch.uint8, device=dr.device)
        before = getattr(self, "debug_flags", 0)
        self.set_debug_flags((before | 0x2) if brute_force else (before & ~0x2))
        try:
            self.check(self.lib.pt_debug_trace_closest(self.handle, C.c_void_p(dr.data_ptr()), len(rays), C.c_void_p(dh.data_ptr())))
            self.sync()
        finally:
            self.set_debug_flags(before)
        return dh.cpu().numpy()[:len(rays) * 32].view(CLOSEST_HIT).copy()

    def trace_ray(self, ray8, log_words=4 * 4096):
        """pt_debug_trace_ray: one host ray (origin, tmin, direction, tmax) through the one-lane two-level walk with its step log. Returns
        the steps written as an [n, 4] uint32 array of (code, a, b, sp) (csrc/pt_trace2.hpp trace_single names the codes; 7 ends a walk).
        A log that fills log_words ends without its code 7: the walk itself still ran to its end. Refuses like the C call does: without
        a top level, PtError; a ray that is not eight floats, PtInvalidArgument."""
        ray = np.ascontiguousarray(ray8, np.float32).reshape(-1)
        if ray.size != 8 or log_words < 4:
            raise PtInvalidArgument("trace_ray takes one ray of eight floats and room for at least one step")
        log = np.zeros(int(log_words), np.uint32)
        self.check(self.lib.pt_debug_trace_ray(self.handle, C.c_void_p(ray.ctypes.data), C.c_void_p(log.ctypes.data), int(log_words)))
        steps = log[:4 * (int(log_words) // 4)].reshape(-1, 4)
        return steps[:int(np.count_nonzero(steps[:, 0]))].copy()

    def accel_stats(self):
        s = AccelStats()
        self.check(self.lib.pt_get_accel_stats(self.handle, C.byref(s)))
        return s

    # multi-GPU gather (pt_comm.hip) ------------------------------------------------------------
    @staticmethod
    def comm_unique_id():
        """ncclGetUniqueId through the library: 128 bytes, made by one rank, handed to the others by the caller."""
        lib = load_library()
        buf = (C.c_uint8 * 128)()
        st = lib.pt_comm_get_unique_id(buf)
        if st != 0:
            raise PtError(f"pt_comm_get_unique_id failed ({st}): {lib.pt_last_error(None).decode()}")
        return bytes(buf)

    def comm_init(self, unique_id, rank, world):
        buf = (C.c_uint8 * 128).from_buffer_copy(unique_id)
        self.check(self.lib.pt_comm_init(self.handle, buf, rank, world))

    def gather_bands(self, local, dst_full, width, height, pixel_bytes, root=0):
        """local / dst_full: CUDA tensors (dst_full may be None on a non-root rank)."""
        self.check(self.lib.pt_gather_bands(self.handle, C.c_void_p(local.data_ptr()),
                                            C.c_void_p(dst_full.data_ptr() if dst_full is not None else None), width, height, pixel_bytes, root))

    def set_sharding(self, rank, world, band=16):
        s = Sharding(rank, world, band, 0)
        self.check(self.lib.pt_set_sharding(self.handle, C.byref(s)))
        self.sharding = (rank, world, band)


def _torch():
    import torch
    if not torch.cuda.is_available():
        raise PtError("no GPU visible to torch: the path tracer has no CPU fallback")
    return torch


def to_device(arr, device):
    """numpy array (any dtype, incl. structured) -> uint8 CUDA tensor holding the same bytes."""
    torch = _torch()
    raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
    if raw.size == 0:
        raw = np.zeros(16, np.uint8)
    return torch.from_numpy(raw.copy()).to(device)


def _download_counted(ctx, fn, dtype, *lead, counts=1):
    """The two calls of a counted download (pt_*_download_*): ask for the counts, then fetch that many records. The result has one axis
    per count. lead: the arguments between the context and the destination."""
    n = [C.c_uint32(0) for _ in range(counts)]
    refs = [C.byref(v) for v in n]
    ctx.check(fn(ctx.handle, *lead, None, 0, *refs))
    out = np.zeros(tuple(v.value for v in n), dtype)
    if out.size:
        ctx.check(fn(ctx.handle, *lead, C.c_void_p(out.ctypes.data), out.size, *refs))
    return out


class SharedScene:
    """A second context's view of a Scene built on another context of the same GPU (pt_share_scene): frames in flight on separate
    streams render one copy of the scene. Holds a reference to the owning Scene so that it outlives the view."""

    def __init__(self, ctx, owner):
        self.ctx, self.owner, self.desc, self.device = ctx, owner, owner.desc, owner.device
        ctx.check(ctx.lib.pt_share_scene(ctx.handle, owner.ctx.handle))

    def GetTopLevelAccelerationStructure(self):
        return self.ctx.handle

    def close(self):
        pass


class Scene:
    """Device-side scene: the part of Scene (Source/Scene.ixx:75-403) and App::UpdateScene
    (Source/App.cpp:1016-1074) that feeds the hot path: vertex/index buffers, descriptor heap,
    ObjectData / InstanceData buffers, BLAS per mesh node, TLAS over instances."""
    SKIN_STAGING_RING = 4          # pinned staging buffers of the joint matrices, taken in turn (SkinSkeletalMeshes)

    def __init__(self, ctx, scene, device=None):
        torch = _torch()
        self.ctx, self.desc = ctx, scene
        self.device = device or torch.device("cuda", ctx.device_ordinal)
        lib = ctx.lib
        self._buffers = []
        ctx.check(lib.pt_heap_resize(ctx.handle, len(scene.heap)))
        heap_dev = []
        for i, item in enumerate(scene.heap):
            t = to_device(item.array, self.device)
            self._buffers.append(t); heap_dev.append(t)
            if item.kind == 0:
                ctx.check(lib.pt_heap_set_buffer(ctx.handle, i, C.c_void_p(t.data_ptr()), item.array.nbytes, item.stride))
            else:
                ctx.check(lib.pt_heap_set_texture(ctx.handle, i, C.c_void_p(t.data_ptr()), item.width, item.height, item.fmt,
                                                  1 if item.kind == 2 else 0))
        self.object_data = to_device(scene.object_data, self.device)
        self.instance_data = to_device(scene.instance_data, self.device)
        ctx.check(lib.pt_set_object_data(ctx.handle, C.c_void_p(self.object_data.data_ptr()), len(scene.object_data)))
        ctx.check(lib.pt_set_instance_data(ctx.handle, C.c_void_p(self.instance_data.data_ptr()), len(scene.instance_data)))
        self._heap_dev = heap_dev
        self.blas_ids = []
        self._skin_cache = {}
        self._skeletal_dev = {}           # Animate: the skeletal vertices of a skinned mesh, uploaded once
        self.CreateAccelerationStructures()

    def close(self):
        """~Scene (Source/Scene.ixx:108-123): the bottom levels this scene built go back to the context. The live top level
        dies with them: a render before the next scene's build answers PT_ERROR_NOT_READY."""
        ctx = self.ctx
        if getattr(ctx, "handle", None):
            for bid in self.blas_ids:
                ctx.lib.pt_release_bottom_level(ctx.handle, bid)
        self.blas_ids = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _geometry_descs(self, node_index):
        """D3D12_RAYTRACING_GEOMETRY_DESC per mesh of a mesh node + the build flags of Scene.ixx:320-329: OPAQUE iff the mesh
        has no material or AlphaMode::Opaque; skeletal mesh nodes are built PREFER_FAST_BUILD | ALLOW_UPDATE, static ones
        PREFER_FAST_TRACE."""
        scene = self.desc
        first, count = scene.blas[node_index]
        geoms = (GeometryDesc * max(1, count))()
        skeletal = False
        for g in range(count):
            mesh, hv, hi = scene.geometry[first + g]
            d = geoms[g]
            d.VertexBuffer = self._heap_dev[hv].data_ptr()
            d.VertexCount, d.VertexStride = len(mesh.vertices), mesh.vertices.dtype.itemsize
            d.IndexBuffer = self._heap_dev[hi].data_ptr()
            d.IndexCount, d.IndexStride = mesh.indices.size, mesh.indices.dtype.itemsize
            alpha_mode = int(mesh.material["AlphaMode"]) if mesh.material is not None else 0
            d.Flags = 1 if alpha_mode == 0 else 0
            skeletal = skeletal or getattr(mesh, "skeletal_vertices", None) is not None
        return geoms, count, (0x8 | 0x1) if skeletal else 0x4

    def SkinSkeletalMeshes(self, mesh, skeletal_transforms):
        """Scene::SkinSkeletalMeshes (Source/Scene.ixx:233-280) for one mesh: joint transforms -> SkeletalMeshSkinning."""
        ctx, lib = self.ctx, self.ctx.lib
        hv = next(h for m, h, _ in self.desc.geometry if m is mesh)
        hm = int(self.desc._motion_heap[id(mesh)])
        torch = _torch()
        if id(mesh) not in self._skin_cache:                     # skeletal vertices once; joint matrices: a ring of pinned staging tensors
            n = int(np.asarray(skeletal_transforms).size)         # + a device tensor that live as long as the scene (no allocation per frame)
            ring = [[torch.zeros(n, dtype=torch.float32).pin_memory(), None] for _ in range(self.SKIN_STAGING_RING)]
            self._skin_cache[id(mesh)] = [to_device(mesh.skeletal_vertices, self.device), ring,
                                          torch.zeros(n, dtype=torch.float32, device=self.device), 0]
        entry = self._skin_cache[id(mesh)]
        sk, ring, tr = entry[0], entry[1], entry[2]
        slot = ring[entry[3] % len(ring)]; entry[3] += 1
        # The host may run frames ahead of the stream (nothing on the dynamic path synchronises): a pinned buffer is rewritten only after
        # the H2D copy that last read it has run -- the event recorded behind that copy. With the ring that wait is over before it starts
        # unless the host is a whole ring ahead. The device tensor needs no ring: copy N+1 is stream-ordered behind skin kernel N.
        staging = slot[0]
        if slot[1] is not None:
            slot[1].synchronize()
        staging.copy_(torch.from_numpy(np.ascontiguousarray(skeletal_transforms, np.float32).reshape(-1)))
        tr.copy_(staging, non_blocking=True)
        if slot[1] is None:
            slot[1] = torch.cuda.Event()
        slot[1].record(torch.cuda.current_stream(self.device))
        ctx.check(lib.pt_skin_mesh(ctx.handle, C.c_void_p(sk.data_ptr()), C.c_void_p(tr.data_ptr()),
                                   C.c_void_p(self._heap_dev[hv].data_ptr()), C.c_void_p(self._heap_dev[hm].data_ptr()), len(mesh.vertices)))

    def UpdateAccelerationStructures(self, node_index):
        """the PERFORM_UPDATE branch of Scene::CreateAccelerationStructures (Source/Scene.ixx:327-345) + TLAS rebuild."""
        ctx, lib = self.ctx, self.ctx.lib
        geoms, count, flags = self._geometry_descs(node_index)
        ctx.check(lib.pt_update_bottom_level(ctx.handle, self.blas_ids[node_index], C.addressof(geoms), count, flags))
        self._build_top_level()

    def download(self, heap_index, dtype):
        return self._heap_dev[heap_index].cpu().numpy().view(dtype)

    def CreateAccelerationStructures(self):
        """Scene::CreateAccelerationStructures (Source/Scene.ixx:286-380)."""
        ctx, scene, lib = self.ctx, self.desc, self.ctx.lib
        for bid in self.blas_ids:
            ctx.check(lib.pt_release_bottom_level(ctx.handle, bid))
        self.blas_ids = []
        for node_index in range(len(scene.blas)):             # one BLAS per MeshNode, one geometry per Mesh
            geoms, count, flags = self._geometry_descs(node_index)
            bid = C.c_uint64(0)
            ctx.check(lib.pt_build_bottom_level(ctx.handle, C.addressof(geoms), count, flags, C.byref(bid)))
            self.blas_ids.append(bid.value)
        self._build_top_level()

    def _build_top_level(self, posed=None):
        """posed: the from_device bytes of pt_build_top_level_posed (Animate), or None: pt_build_top_level. instance descs as Scene::CreateAccelerationStructures fills them (Scene.ixx:365-377). The array is kept: a dynamic frame
        re-submits it as it is (transforms of the static instances do not move; update_instance_transform() for those that do)."""
        ctx, scene, lib = self.ctx, self.desc, self.ctx.lib
        n = len(scene.objects)
        if getattr(self, "_descs", None) is None or len(self._descs) != max(1, n) or self._descs_ids != list(self.blas_ids):
            descs = (InstanceDesc * max(1, n))()
            tr = np.ascontiguousarray(scene.instance_data["ObjectToWorld"], np.float32).reshape(n, 12) if n else np.zeros((0, 12), np.float32)
            for i in range(n):
                descs[i].Transform = (C.c_float * 12)(*tr[i].tolist())
                descs[i].InstanceID = int(scene.instance_ids[i])
                descs[i].InstanceMask = int(scene.instance_masks[i])
                descs[i].AccelerationStructure = self.blas_ids[int(scene.instance_blas[i])]
            self._descs, self._descs_ids = descs, list(self.blas_ids)
        if posed is not None:
            ctx.check(lib.pt_build_top_level_posed(ctx.handle, C.addressof(self._descs), n, 0x4, C.c_void_p(self.instance_data.data_ptr()),
                                                   C.c_void_p(posed.ctypes.data)))
            return
        ctx.check(lib.pt_build_top_level(ctx.handle, C.addressof(self._descs), n, 0x4))

    def GetTopLevelAccelerationStructure(self):
        return self.ctx.handle        # the context owns the single TLAS

    def Animate(self, animation):
        """One dynamic frame's update in the reference's order (Scene::Tick -> Refresh -> SkinSkeletalMeshes -> CreateAccelerationStructures,
        Source/Scene.ixx:174-188, 195-380), all of it enqueued on the stream, nothing computed or copied by the host but the few bytes of
        the states: pt_anim_evaluate poses every animated object at its current time (joint matrices and InstanceData on the device),
        pt_skin_mesh reads the joint matrices where the pose left them, the skinned mesh nodes are refitted, and the top level takes the
        posed instances' transforms from the device."""
        ctx, lib = self.ctx, self.ctx.lib
        animation.Evaluate(self.instance_data)
        for obj, handle in zip(animation.objects, animation.handles):
            for k, skin in enumerate(obj.skins):
                if skin.scene_node is None:
                    continue
                ptr, count = animation.skeletal_transforms(handle, k)
                for mesh in self.desc.nodes[skin.scene_node].meshes:
                    if mesh.skeletal_vertices is None:
                        continue
                    if id(mesh) not in self._skeletal_dev:
                        self._skeletal_dev[id(mesh)] = to_device(mesh.skeletal_vertices, self.device)
                    hv = next(h for m, h, _ in self.desc.geometry if m is mesh)
                    hm = int(self.desc._motion_heap[id(mesh)])
                    ctx.check(lib.pt_skin_mesh(ctx.handle, C.c_void_p(self._skeletal_dev[id(mesh)].data_ptr()), C.c_void_p(ptr),
                                               C.c_void_p(self._heap_dev[hv].data_ptr()), C.c_void_p(self._heap_dev[hm].data_ptr()), len(mesh.vertices)))
        for node_index in animation.skinned_nodes:
            geoms, count, flags = self._geometry_descs(node_index)
            ctx.check(lib.pt_update_bottom_level(ctx.handle, self.blas_ids[node_index], C.addressof(geoms), count, flags))
        self._build_top_level(posed=animation.from_device(len(self.desc.objects)))


def _vp(a):
    return C.c_void_p(a.ctypes.data) if a is not None and a.size else None


class Animation:
    """The animated render objects of a scene (scenes.AnimatedObject) on the device: one rig per animation file (shared by the objects
    that name it), one animated object per render object -- the reference binds a copy of the AnimationCollection to every render
    object (Source/Scene.ixx:165-168) --, and per object the selected clip and its time, as Animation::m_time
    (Source/Animation.ixx:104-113). Nothing here computes a matrix: Scene.Animate hands the times to the device."""

    def __init__(self, ctx, objects):
        """ctx None: the clock alone (clips and times), nothing on a device."""
        self.ctx, self.objects = ctx, list(objects)
        lib = ctx.lib if ctx is not None else None
        self.rigs, self.handles = {}, []
        for o in (self.objects if ctx is not None else []):
            r = o.rig
            if id(r) not in self.rigs:
                n = len(r.parents)
                arrays = (np.ascontiguousarray(r.parents, np.int32), np.ascontiguousarray(r.rest, np.float32).reshape(n, 10),
                          np.ascontiguousarray(r.durations, np.float64), np.ascontiguousarray(r.channels, np.uint32).reshape(len(r.durations), n, 3, 2),
                          np.ascontiguousarray(r.key_times, np.float32), np.ascontiguousarray(r.key_values, np.float32).reshape(-1, 4))
                h = C.c_uint64(0)
                ctx.check(lib.pt_anim_create_rig(ctx.handle, n, _vp(arrays[0]), _vp(arrays[1]), len(arrays[2]), _vp(arrays[2]), _vp(arrays[3]),
                                                 _vp(arrays[4]), _vp(arrays[5]), len(arrays[4]), C.byref(h)))
                self.rigs[id(r)] = h.value
            bn = np.ascontiguousarray(o.binding_nodes, np.uint32); bi = np.ascontiguousarray(o.binding_instances, np.uint32)
            bg = np.ascontiguousarray(o.binding_globals, np.float32).reshape(len(bn), 16)
            sn = np.array([s.mesh_node for s in o.skins], np.uint32); sc = np.array([len(s.joint_nodes) for s in o.skins], np.uint32)
            jn = np.concatenate([np.asarray(s.joint_nodes, np.uint32) for s in o.skins]) if o.skins else np.zeros(0, np.uint32)
            ib = (np.concatenate([np.asarray(s.inverse_binds, np.float32).reshape(-1, 16) for s in o.skins]) if o.skins else np.zeros((0, 16), np.float32))
            tr = np.ascontiguousarray(o.transform, np.float32).reshape(16)
            h = C.c_uint64(0)
            ctx.check(lib.pt_anim_create_object(ctx.handle, self.rigs[id(o.rig)], _vp(tr), len(bn), _vp(bn), _vp(bi), _vp(bg), len(sn), _vp(sn), _vp(sc),
                                                _vp(jn), _vp(np.ascontiguousarray(ib)), C.byref(h)))
            self.handles.append(h.value)
        self.clips = [min(int(o.clip), len(o.rig.durations) - 1) for o in self.objects]      # AnimationCollection::GetSelectedIndex
        self.times = [0.0] * len(self.objects)
        self.skinned_nodes = sorted({s.scene_node for o in self.objects for s in o.skins if s.scene_node is not None})
        self._states = (AnimState * max(1, len(self.objects)))()
        self._from_device = None

    def duration(self, i):
        return float(self.objects[i].rig.durations[self.clips[i]])

    def SetSelectedIndex(self, i, clip):
        self.clips[i] = min(int(clip), len(self.objects[i].rig.durations) - 1)

    def SetTime(self, seconds=0.0, index=None):
        """Animation::SetTime: clamp(seconds, 0, duration), for one object or for all."""
        for i in (range(len(self.objects)) if index is None else [index]):
            self.times[i] = min(max(float(seconds), 0.0), self.duration(i))

    def Tick(self, elapsed_seconds, index=None):
        """Animation::Tick: time = fmod(time + elapsed, duration). A clip of duration 0 stays at time 0 (the reference's fmod yields NaN)."""
        import math
        for i in (range(len(self.objects)) if index is None else [index]):
            d = self.duration(i)
            self.times[i] = math.fmod(self.times[i] + float(elapsed_seconds), d) if d > 0.0 else 0.0

    def Evaluate(self, device_instances=None):
        """pt_anim_evaluate of every object at its clip and time. device_instances: the scene's InstanceData tensor, or None."""
        for i, h in enumerate(self.handles):
            self._states[i].Object, self._states[i].Clip, self._states[i].Time = h, self.clips[i], self.times[i]
        self.ctx.check(self.ctx.lib.pt_anim_evaluate(self.ctx.handle, C.addressof(self._states), len(self.handles),
                                                     C.c_void_p(device_instances.data_ptr()) if device_instances is not None else None))

    def from_device(self, instance_count):
        """The from_device bytes of pt_build_top_level_posed: 1 for every instance an object's bindings pose."""
        if self._from_device is None or len(self._from_device) != max(1, instance_count):
            m = np.zeros(max(1, instance_count), np.uint8)
            for o in self.objects:
                m[np.asarray(o.binding_instances, np.int64)] = 1
            self._from_device = m
        return self._from_device

    def skeletal_transforms(self, handle, skin):
        """(device pointer, joint count) of a skin's float3x4 matrices: what pt_skin_mesh takes."""
        p, n = C.c_void_p(), C.c_uint32(0)
        self.ctx.check(self.ctx.lib.pt_anim_skeletal_transforms(self.ctx.handle, handle, skin, C.byref(p), C.byref(n)))
        return p.value, n.value

    def _download(self, fn, shape, *lead):
        n = C.c_uint32(0)
        self.ctx.check(fn(self.ctx.handle, *lead, None, 0, C.byref(n)))
        out = np.zeros((n.value,) + shape, np.float32)
        if n.value:
            self.ctx.check(fn(self.ctx.handle, *lead, C.c_void_p(out.ctypes.data), n.value, C.byref(n)))
        return out

    def download_globals(self, i):
        """The global transforms of object i's last evaluation, [nodes, 4, 4] float32 (row-vector convention). Synchronises."""
        return self._download(self.ctx.lib.pt_anim_download_globals, (4, 4), self.handles[i])

    def download_skeletal(self, i, skin):
        """A skin's float3x4 matrices as the last evaluation left them, [joints, 3, 4] float32. Synchronises."""
        return self._download(self.ctx.lib.pt_anim_download_skeletal, (3, 4), self.handles[i], skin)

    def close(self):
        ctx = self.ctx
        if getattr(ctx, "handle", None):
            for h in self.handles:
                ctx.lib.pt_anim_release_object(ctx.handle, h)
            for h in self.rigs.values():
                ctx.lib.pt_anim_release_rig(ctx.handle, h)
        self.handles, self.rigs = [], {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def debug_slerp(ctx, q0, q1, t):
    """pt_anim_debug_slerp: the device's slerp on host cases; [n, 12] float32 (result, then c, x, s, w, a0, a1, sin a0, sin a1)."""
    q0 = np.ascontiguousarray(q0, np.float32).reshape(-1, 4); q1 = np.ascontiguousarray(q1, np.float32).reshape(-1, 4)
    t = np.ascontiguousarray(t, np.float32).reshape(-1)
    out = np.zeros((len(t), 12), np.float32)
    ctx.check(ctx.lib.pt_anim_debug_slerp(ctx.handle, _vp(q0), _vp(q1), _vp(t), len(t), _vp(out)))
    return out


def alloc_textures(width, local_rows_, device, with_f32=False, with_denoiser_outputs=False):
    """The G-buffer textures of App::CreateWindowSizeDependentResources (Source/App.cpp:438-455) as
    linear CUDA tensors in the same DXGI formats."""
    torch = _torch()
    out = {}
    tmap = {"<f4": torch.float32, "<i2": torch.int16, "<u2": torch.int16, "u1": torch.uint8}
    for name, (dt, ch) in L.GBUFFER_FORMATS.items():
        out[name] = torch.zeros((local_rows_, width, ch), dtype=tmap[dt], device=device)
    if with_f32:
        out["RadianceF32"] = torch.zeros((local_rows_, width, 4), dtype=torch.float32, device=device)
    if with_denoiser_outputs:
        for name, (dt, ch) in L.DENOISER_FORMATS.items():
            out[name] = torch.zeros((local_rows_, width, ch), dtype=tmap[dt], device=device)
    return out


def alloc_post_textures(width, height, device):
    """The outputs of the post-processing chain as linear CUDA tensors: Color (R16G16B16A16_FLOAT), BackBuffer (R10G10B10A2_UNORM,
    one 32-bit word per pixel), Display8 (R8G8B8A8_UNORM)."""
    torch = _torch()
    tmap = {"<u2": torch.int16, "<u4": torch.int32, "u1": torch.uint8}
    return {name: torch.zeros((height, width, ch) if ch > 1 else (height, width), dtype=tmap[dt], device=device)
            for name, (dt, ch) in L.POST_FORMATS.items()}


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _pack_textures(tex):
    t = Textures()
    for n in TEXTURE_NAMES:
        v = tex.get(n) if tex else None
        setattr(t, n, v.data_ptr() if v is not None else None)
    return t


def textures_to_numpy(tex):
    out = {}
    for name, t in tex.items():
        a = t.detach().cpu().numpy()
        base = name[len("Previous"):] if name in L.DI_PREVIOUS_TEXTURES else name
        if base in L.GBUFFER_FORMATS:
            a = a.view(np.dtype(L.GBUFFER_FORMATS[base][0]))
        elif name in L.DENOISER_FORMATS:
            a = a.view(np.dtype(L.DENOISER_FORMATS[name][0]))
        elif name in L.POST_FORMATS:
            a = a.view(np.dtype(L.POST_FORMATS[name][0]))
        out[name] = a
    return out


class GBufferGeneration:
    """Mirror of `struct GBufferGeneration` (Source/GBufferGeneration.ixx:27-122)."""
    Flags = L.GBufferFlags

    def __init__(self, ctx):
        self.ctx = ctx
        self.GPUBuffers = {"SceneData": None, "Camera": None, "InstanceData": None, "ObjectData": None}
        self.Textures = {}

    def Render(self, topLevelAccelerationStructure, constants):
        """constants: numpy GBUFFER_CONSTANTS {RenderSize, Flags}. GPUBuffers.Camera / SceneData are the
        host structs (numpy CAMERA / SCENE_DATA) the reference copies into its constant buffers."""
        ctx, lib = self.ctx, self.ctx.lib
        cam = np.array(self.GPUBuffers["Camera"]); sd = np.array(self.GPUBuffers["SceneData"])
        ctx.check(lib.pt_set_camera(ctx.handle, C.c_void_p(cam.ctypes.data)))
        ctx.check(lib.pt_set_scene_data(ctx.handle, C.c_void_p(sd.ctypes.data)))
        k = np.array(constants).reshape(())
        t = _pack_textures(self.Textures)
        ctx.check(lib.pt_gbuffer_render(ctx.handle, C.c_void_p(k.ctypes.data), C.addressof(t)))


class Raytracing:
    """Mirror of `struct Raytracing` (Source/Raytracing.ixx:29-250), DEFAULT permutation."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.GPUBuffers = {"SceneData": None, "Camera": None, "ObjectData": None}
        self.Textures = {}
        self._settings = None

    def SetConstants(self, graphicsSettings):
        self._settings = np.array(graphicsSettings).reshape(())
        self.ctx.check(self.ctx.lib.pt_raytrace_set_constants(self.ctx.handle, C.c_void_p(self._settings.ctypes.data)))

    def Render(self, topLevelAccelerationStructure):
        ctx, lib = self.ctx, self.ctx.lib
        cam = np.array(self.GPUBuffers["Camera"]); sd = np.array(self.GPUBuffers["SceneData"])
        ctx.check(lib.pt_set_camera(ctx.handle, C.c_void_p(cam.ctypes.data)))
        ctx.check(lib.pt_set_scene_data(ctx.handle, C.c_void_p(sd.ctypes.data)))
        t = _pack_textures(self.Textures)
        ctx.check(lib.pt_raytrace_render(ctx.handle, C.addressof(t)))


def onion_table(which):
    """The static tables of the ReGIR Onion layout at unit scale (pt_di_regir_onion_table; host only, no context, no GPU), float32.
    which = 0: the 16 squared layer boundaries; 1: the 20 ring thresholds, by group; 2: the 241 azimuth thresholds, by (group, ring);
    3: the cell spheres [2253, 4] (centre xyz, radius)."""
    lib = load_library()
    n = C.c_uint32(0)
    if lib.pt_di_regir_onion_table(which, None, 0, C.byref(n)) != 0:
        raise PtInvalidArgument("pt_di_regir_onion_table: which must be 0..3")
    out = np.empty(n.value, np.float32)
    if lib.pt_di_regir_onion_table(which, C.c_void_p(out.ctypes.data), n.value, C.byref(n)) != 0:
        raise PtInvalidArgument("pt_di_regir_onion_table failed")
    return out.reshape(-1, 4) if which == 3 else out


class DirectLighting:
    """Mirror of the reference's RTXDI operator (Source/RTXDI.ixx: SetConstants + Render) for this library's DI pass: emissive-triangle
    lights, LocalLightSamples power-proportional candidates, streaming RIS, one visibility ray. Writes Textures["Diffuse"] /
    Textures["Specular"] (or adds to Textures["Radiance"] when it is the last render pass with Denoiser None / DLSS-RR)."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.GPUBuffers = {"SceneData": None, "Camera": None, "ObjectData": None}
        self.Textures = {}
        self._settings = None

    def SetConstants(self, settings):
        self._settings = np.array(settings).reshape(())
        self.ctx.check(self.ctx.lib.pt_di_set_constants(self.ctx.handle, C.c_void_p(self._settings.ctypes.data)))

    def Render(self, topLevelAccelerationStructure):
        ctx, lib = self.ctx, self.ctx.lib
        if self.GPUBuffers["Camera"] is not None:
            cam = np.array(self.GPUBuffers["Camera"])
            ctx.check(lib.pt_set_camera(ctx.handle, C.c_void_p(cam.ctypes.data)))
        if self.GPUBuffers["SceneData"] is not None:
            sd = np.array(self.GPUBuffers["SceneData"])
            ctx.check(lib.pt_set_scene_data(ctx.handle, C.c_void_p(sd.ctypes.data)))
        t = _pack_textures(self.Textures)
        if any(self.Textures.get(n) is not None for n in L.DI_PREVIOUS_TEXTURES):
            p = PreviousTextures(*[_ptr(self.Textures.get(n)) for n in L.DI_PREVIOUS_TEXTURES])
            ctx.check(lib.pt_di_render_with_history(ctx.handle, C.addressof(t), C.addressof(p)))
        else:
            ctx.check(lib.pt_di_render(ctx.handle, C.addressof(t)))

    def SetResampling(self, settings):
        """PtDIResamplingSettings (layouts.di_resampling_settings), or None: the plain pass. A changed value resets the history."""
        if settings is None:
            self.ctx.check(self.ctx.lib.pt_di_set_resampling(self.ctx.handle, None))
            return
        self._resampling = np.array(settings).reshape(())
        self.ctx.check(self.ctx.lib.pt_di_set_resampling(self.ctx.handle, C.c_void_p(self._resampling.ctypes.data)))

    def ResetHistory(self):
        self.ctx.check(self.ctx.lib.pt_di_reset_history(self.ctx.handle))

    def SetLightSampling(self, settings):
        """PtDILightSamplingSettings (layouts.di_light_sampling_settings), or None: the power CDF. A changed value resets the history."""
        if settings is None:
            self.ctx.check(self.ctx.lib.pt_di_set_light_sampling(self.ctx.handle, None))
            return
        self._light_sampling = np.array(settings).reshape(())
        self.ctx.check(self.ctx.lib.pt_di_set_light_sampling(self.ctx.handle, C.c_void_p(self._light_sampling.ctypes.data)))

    def SetVisibility(self, settings):
        """PtDIVisibilitySettings (layouts.di_visibility_settings), or None: no visibility in the reservoirs. It acts only with reservoir
        reuse on. A changed value resets the history."""
        if settings is None:
            self.ctx.check(self.ctx.lib.pt_di_set_visibility(self.ctx.handle, None))
            return
        self._visibility = np.array(settings).reshape(())
        self.ctx.check(self.ctx.lib.pt_di_set_visibility(self.ctx.handle, C.c_void_p(self._visibility.ctypes.data)))

    def SetPairwise(self, settings):
        """PtDIPairwiseSettings (layouts.di_pairwise_settings), or None: off. A flag turns the Basic bias correction of its pass into
        Pairwise. A changed value resets the history."""
        if settings is None:
            self.ctx.check(self.ctx.lib.pt_di_set_pairwise(self.ctx.handle, None))
            return
        self._pairwise = np.array(settings).reshape(())
        self.ctx.check(self.ctx.lib.pt_di_set_pairwise(self.ctx.handle, C.c_void_p(self._pairwise.ctypes.data)))

    def SetReGIRLayout(self, settings):
        """PtDIReGIRLayoutSettings (layouts.di_regir_layout_settings), or None: the Grid. It acts only in ReGIR mode. A changed value
        resets the history."""
        if settings is None:
            self.ctx.check(self.ctx.lib.pt_di_set_regir_layout(self.ctx.handle, None))
            return
        self._regir_layout = np.array(settings).reshape(())
        self.ctx.check(self.ctx.lib.pt_di_set_regir_layout(self.ctx.handle, C.c_void_p(self._regir_layout.ctypes.data)))

    def SetBrdfSampling(self, settings):
        """layouts.di_brdf_settings (BrdfSamples, BrdfCutoff), or None: no BRDF candidates in initial sampling (0 samples). A changed
        value resets the history; a refused one leaves the previous setting active."""
        if settings is None:
            self.ctx.check(self.ctx.lib.pt_di_set_brdf_sampling(self.ctx.handle, 0, 0.0))
            return
        s = np.array(settings).reshape(())
        self.ctx.check(self.ctx.lib.pt_di_set_brdf_sampling(self.ctx.handle, int(s["BrdfSamples"]), float(s["BrdfCutoff"])))

    def SetPdfMipmap(self, enabled):
        """True: every Render builds the local-light PDF texture and its mip chain, and in the Power_RIS / ReGIR modes the light tiles
        come from a descent of the chain (pt_di_set_pdf_mipmap). False, the default: the power prefix sum. A changed value resets the
        history."""
        self.ctx.check(self.ctx.lib.pt_di_set_pdf_mipmap(self.ctx.handle, 1 if enabled else 0))

    def download_pdf_texture(self):
        """The levels of the PDF texture of the last Render: a list of float32 arrays [height, width], level 0 first; empty when that
        render built none. Synchronises."""
        ctx, fn = self.ctx, self.ctx.lib.pt_di_download_pdf_texture
        levels = []
        while len(levels) < 16:
            w, h = C.c_uint32(0), C.c_uint32(0)
            ctx.check(fn(ctx.handle, len(levels), None, 0, C.byref(w), C.byref(h)))
            if w.value == 0 or h.value == 0:
                break
            out = np.zeros((h.value, w.value), np.float32)
            ctx.check(fn(ctx.handle, len(levels), C.c_void_p(out.ctypes.data), out.size, C.byref(w), C.byref(h)))
            levels.append(out)
        return levels

    def download_brdf_candidates(self):
        """The BRDF candidates of the last Render (numpy layouts.DI_BRDF_CANDIDATE, [local pixels * BrdfSamples], pixel-major; empty
        when that render drew none)."""
        return _download_counted(self.ctx, self.ctx.lib.pt_di_download_brdf_candidates, L.DI_BRDF_CANDIDATE)

    def download_presampled(self, which):
        """which = 0: the Power_RIS tiles (128 x 1024, tile-major), 1: the ReGIR cells (cell-major; Grid: 4096 x 512, x fastest; Onion:
        2253 x 512 in the layout's cell order) of the last Render (numpy layouts.DI_PRESAMPLED_LIGHT; empty when that render did not
        fill them)."""
        return _download_counted(self.ctx, self.ctx.lib.pt_di_download_presampled, L.DI_PRESAMPLED_LIGHT, which)

    def download_reservoirs(self):
        """The final reservoirs of the last Render (numpy layouts.DI_RESERVOIR, row-major pixels; empty without reuse)."""
        return _download_counted(self.ctx, self.ctx.lib.pt_di_download_reservoirs, L.DI_RESERVOIR)

    def light_count(self):
        n = C.c_uint32(0)
        self.ctx.check(self.ctx.lib.pt_di_light_count(self.ctx.handle, C.byref(n)))
        return n.value

    def download_lights(self):
        """The light records of the last Render (numpy layouts.TRIANGLE_LIGHT, list order)."""
        return _download_counted(self.ctx, self.ctx.lib.pt_di_download_lights, L.TRIANGLE_LIGHT)


def pdf_texture_size(n):
    """(width, height, mip_levels) of the local-light PDF texture of n lights (pt_di_pdf_texture_size; host only, no context, no GPU)."""
    w, h, m = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    if not 0 <= int(n) <= 0xFFFFFFFF or load_library().pt_di_pdf_texture_size(int(n), C.byref(w), C.byref(h), C.byref(m)) != 0:
        raise PtInvalidArgument("pt_di_pdf_texture_size: the light count must be 0..2^24")
    return w.value, h.value, m.value


class MipmapGeneration:
    """Mirror of `struct MipmapGeneration` (Source/MipmapGeneration.ixx: SetTexture + Process) for an R32_FLOAT texture. SetTexture takes
    the levels, level 0 first, as float32 device tensors or device addresses (level k: max(1, width >> k) x max(1, height >> k), row-major);
    Process reads level 0 and writes the others on the context's stream. No scene is needed."""

    def __init__(self, ctx):
        self.ctx = ctx
        self._levels, self._size = None, (0, 0)

    def SetTexture(self, levels, width, height):
        self._levels, self._size = list(levels), (int(width), int(height))

    def Process(self):
        if self._levels is None:
            raise PtInvalidArgument("MipmapGeneration.Process: call SetTexture first")
        addresses = [v if isinstance(v, int) else (_ptr(v) or 0) for v in self._levels]
        table = (C.c_void_p * max(len(addresses), 1))(*addresses)
        self.ctx.check(self.ctx.lib.pt_mipmap_generate(self.ctx.handle, C.cast(table, C.c_void_p), self._size[0], self._size[1], len(addresses)))


class PostProcessing:
    """App::PostProcessGraphics with Denoiser::None (Source/App.cpp:1506-1571): Bloom + Merge, ToneMap, CopyTexture. SetConstants takes
    PtPostProcessSettings (layouts.post_processing_settings); Render reads Textures["Radiance"] and writes whichever of Color / BackBuffer /
    Display8 are bound. Runs on the full frame: a sharded host calls it on the gathered frame. No scene is needed."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.Textures = {}
        self._settings = None

    def SetConstants(self, settings):
        self._settings = np.array(settings).reshape(())
        self.ctx.check(self.ctx.lib.pt_post_set_constants(self.ctx.handle, C.c_void_p(self._settings.ctypes.data)))

    def Render(self, textures=None):
        tex = self.Textures if textures is None else textures
        t = PostTextures(*[_ptr(tex.get(n)) for n in ("Radiance", "Color", "BackBuffer", "Display8")])
        self.ctx.check(self.ctx.lib.pt_post_render(self.ctx.handle, C.addressof(t)))

    def download_bloom(self, stage):
        """The image bloom stage `stage` (0..8) wrote in the last Render with bloom on: uint16 fp16 bits (h, w, 4);
        empty (0, 0, 4) when there was none. Synchronises."""
        w, h = C.c_uint32(0), C.c_uint32(0)
        self.ctx.check(self.ctx.lib.pt_post_download_bloom(self.ctx.handle, stage, None, 0, C.byref(w), C.byref(h)))
        out = np.zeros((h.value, w.value, 4), np.uint16)
        if out.size:
            self.ctx.check(self.ctx.lib.pt_post_download_bloom(self.ctx.handle, stage, C.c_void_p(out.ctypes.data), w.value * h.value,
                                                               C.byref(w), C.byref(h)))
        return out


def nrd_reblur_hit_distance_defaults():
    """pt_nrd_reblur_hit_distance_defaults: nrd::ReblurSettings().hitDistanceParameters as the library states them. No GPU."""
    out = np.zeros(4, np.float32)
    load_library().pt_nrd_reblur_hit_distance_defaults(C.c_void_p(out.ctypes.data))
    return out


class NRDComposition:
    """Mirror of `struct NRDComposition` (Source/NRDComposition.ixx -> Shaders/NRDComposition.hlsl:36-88), the pass App::ProcessNRD
    (Source/App.cpp:1595-1688) runs in front of the denoiser (IsPack = 1) and behind it (IsPack = 0). Process takes the textures by the
    names of layouts.NRD_COMPOSITION_TEXTURES (a missing name is an unbound texture) and PtNRDCompositionConstants
    (layouts.nrd_composition_constants). Element-wise: a sharded context passes its own rows and their size. No scene is needed."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.Textures = {}

    def Process(self, textures, constants):
        """textures: the dict of bound textures, None: self.Textures. constants: one record of layouts.NRD_COMPOSITION_CONSTANTS."""
        tex = self.Textures if textures is None else textures
        k = _nrd_constants(constants)
        t = NRDCompositionTextures(*[_ptr(tex.get(n)) for n in L.NRD_COMPOSITION_TEXTURES])
        self.ctx.check(self.ctx.lib.pt_nrd_composition_process(self.ctx.handle, C.c_void_p(k.ctypes.data), C.addressof(t)))


def _nrd_constants(constants):
    """the 32 bytes the library reads: anything but one record of the mirror's dtype is refused here (its values are the library's to check)"""
    k = np.array(constants)
    if k.dtype != L.NRD_COMPOSITION_CONSTANTS or k.size != 1:
        raise PtInvalidArgument("constants must be one PtNRDCompositionConstants record (layouts.nrd_composition_constants)")
    return np.ascontiguousarray(k).reshape(())


def nrd_composition_pixels_per_lane(pointers, constants):
    """pt_nrd_composition_pixels_per_lane: 2 or 1, the form pt_nrd_composition_process would launch for textures at these addresses
    (pointers: name of layouts.NRD_COMPOSITION_TEXTURES -> device address as an int, a missing name is unbound), 0 if it would refuse
    the call. Host arithmetic: no GPU, nothing is dereferenced."""
    k = _nrd_constants(constants)
    t = NRDCompositionTextures(*[pointers.get(n) for n in L.NRD_COMPOSITION_TEXTURES])
    return load_library().pt_nrd_composition_pixels_per_lane(C.c_void_p(k.ctypes.data), C.addressof(t))


class _Filter:
    """What Denoiser, Upscaler and Reconstruction have in common: the textures by name, the settings record last accepted, the history.
    A subclass names its record (_DTYPE, _RECORD, _LAYOUT for the message) and its two library functions (_SET, _RESET)."""
    _DTYPE = _RECORD = _LAYOUT = _SET = _RESET = None

    def __init__(self, ctx):
        self.ctx = ctx
        self.Textures = {}
        self._settings = None

    def _set_constants(self, settings):
        k = np.array(settings)
        if k.dtype != self._DTYPE or k.size != 1:
            raise PtInvalidArgument(f"settings must be one {self._RECORD} record (layouts.{self._LAYOUT})")
        k = np.ascontiguousarray(k).reshape(())
        self.ctx.check(getattr(self.ctx.lib, self._SET)(self.ctx.handle, C.c_void_p(k.ctypes.data)))
        self._settings = k

    def ResetHistory(self):
        self.ctx.check(getattr(self.ctx.lib, self._RESET)(self.ctx.handle))


class Denoiser(_Filter):
    """The library's own denoiser for the ReLAX slot between the two calls of the NRD composition pass (pt_denoiser_*; DESIGN.md section
    1, "Denoiser"): temporal accumulation with reprojection, a variance estimate, an edge-stopping a-trous wavelet. Not NRD's ReLAX, and
    ReLAX's packing only: SetConstants refuses denoiser=DENOISER_NRD_REBLUR. Process takes the textures by the names of
    layouts.DENOISER_TEXTURES (a missing name is an unbound texture); the Denoised pair may be the Noisy pair. Runs on the full frame: a
    sharded host calls it on the gathered frame. No scene is needed.

    An instance is callable as denoise(noisy_diffuse, noisy_specular) -> (denoised_diffuse, denoised_specular), in place, on the guide
    textures of self.Textures: what Renderer.render(..., nrd=DENOISER_NRD_RELAX, denoise=...) asks for."""
    _DTYPE, _RECORD, _LAYOUT = L.DENOISER_SETTINGS, "PtDenoiserSettings", "denoiser_settings"
    _SET, _RESET = "pt_denoiser_set_constants", "pt_denoiser_reset_history"

    def SetConstants(self, settings, denoiser=L.DENOISER_NRD_RELAX):
        """settings: PtDenoiserSettings (layouts.denoiser_settings). denoiser: the packing of the pair it will be handed."""
        if int(denoiser) != L.DENOISER_NRD_RELAX:
            raise PtInvalidArgument("the denoiser reads ReLAX's packing (radiance, hit distance) only: ReBLUR's (YCoCg, normalised hit "
                                    "distance) and the other Denoiser values are not served")
        self._set_constants(settings)

    def Process(self, textures=None):
        tex = self.Textures if textures is None else textures
        t = DenoiserTextures(*[_ptr(tex.get(n)) for n in L.DENOISER_TEXTURES])
        self.ctx.check(self.ctx.lib.pt_denoiser_process(self.ctx.handle, C.addressof(t)))

    def DownloadHistory(self):
        """The accumulated length of the diffuse channel per pixel after the last Process: float32 (h, w), 0 where the G-buffer missed;
        empty (0, 0) when there is no history. Synchronises."""
        w, h = C.c_uint32(0), C.c_uint32(0)
        self.ctx.check(self.ctx.lib.pt_denoiser_download_history(self.ctx.handle, None, 0, C.byref(w), C.byref(h)))
        out = np.zeros((h.value, w.value), np.float32)
        if out.size:
            self.ctx.check(self.ctx.lib.pt_denoiser_download_history(self.ctx.handle, C.c_void_p(out.ctypes.data), out.size, C.byref(w), C.byref(h)))
        return out

    def __call__(self, noisy_diffuse, noisy_specular):
        if self._settings is None:
            raise PtInvalidArgument("Denoiser: call SetConstants first")
        self.Process(dict(self.Textures, NoisyDiffuse=noisy_diffuse, NoisySpecular=noisy_specular,
                          DenoisedDiffuse=noisy_diffuse, DenoisedSpecular=noisy_specular))
        return noisy_diffuse, noisy_specular


def upscaler_render_size(mode, output_size):
    """pt_upscaler_render_size: the render size (w, h) of a PtSuperResolutionMode (layouts.SUPER_RESOLUTION_*) for an output size. No GPU."""
    out, size = (C.c_uint32 * 2)(), (C.c_uint32 * 2)(*[int(v) for v in output_size])
    if not 0 <= int(mode) <= 0xFFFFFFFF or load_library().pt_upscaler_render_size(int(mode), size, out) != 0:
        raise PtInvalidArgument("mode must be a PtSuperResolutionMode value and output 1..16384 on both axes")
    return out[0], out[1]


def upscaler_jitter(frame_index, render_size, output_size):
    """pt_upscaler_jitter: the Camera.Jitter of frame `frame_index` as two float32, in [-0.5, 0.5). No GPU."""
    out = (C.c_float * 2)()
    render, output = (C.c_uint32 * 2)(*[int(v) for v in render_size]), (C.c_uint32 * 2)(*[int(v) for v in output_size])
    if load_library().pt_upscaler_jitter(int(frame_index), render, output, out) != 0:
        raise PtInvalidArgument("render and output must be 1..16384 on both axes")
    return np.float32(out[0]), np.float32(out[1])


class Upscaler(_Filter):
    """The library's own temporal upscaler for the super-resolution slot between the denoiser and the post chain (pt_upscaler_*;
    DESIGN.md section 1, "Upscaler"): a temporal accumulating upscaler from RenderSize to OutputSize, where the reference loads DLSS or
    XeSS. Not a port of either. Process takes the textures by the names of layouts.UPSCALER_TEXTURES (a missing name is an unbound
    texture) and the Camera.Jitter the frame was rendered with. Runs on the full frame of an unsharded context. No scene is needed."""
    _DTYPE, _RECORD, _LAYOUT = L.UPSCALER_SETTINGS, "PtUpscalerSettings", "upscaler_settings"
    _SET, _RESET = "pt_upscaler_set_constants", "pt_upscaler_reset_history"

    @property
    def settings(self):
        """the PtUpscalerSettings record last accepted, or None"""
        return self._settings

    def SetConstants(self, settings):
        """settings: PtUpscalerSettings (layouts.upscaler_settings)."""
        self._set_constants(settings)

    def Process(self, jitter, textures=None):
        tex = self.Textures if textures is None else textures
        t = UpscalerTextures(*[_ptr(tex.get(n)) for n in L.UPSCALER_TEXTURES])
        j = (C.c_float * 2)(float(jitter[0]), float(jitter[1]))
        self.ctx.check(self.ctx.lib.pt_upscaler_process(self.ctx.handle, C.addressof(t), j))

    def DownloadHistory(self):
        """The accumulated weight n per output pixel after the last Process: float32 (h, w); empty (0, 0) when there is no history.
        Synchronises."""
        w, h = C.c_uint32(0), C.c_uint32(0)
        self.ctx.check(self.ctx.lib.pt_upscaler_download_history(self.ctx.handle, None, 0, C.byref(w), C.byref(h)))
        out = np.zeros((h.value, w.value), np.float32)
        if out.size:
            self.ctx.check(self.ctx.lib.pt_upscaler_download_history(self.ctx.handle, C.c_void_p(out.ctypes.data), out.size, C.byref(w), C.byref(h)))
        return out


class Reconstruction(_Filter):
    """The library's own denoising upscaler for the ray-reconstruction slot of App::PostProcessGraphics (pt_reconstruction_*; DESIGN.md
    section 1, "Ray reconstruction"), where the reference's default settings call DLSS Ray Reconstruction. Not a port of it. From the noisy
    Radiance of a Denoiser = DLSS-RR frame, the two albedos and the G-buffer guides at RenderSize to the denoised Color at OutputSize.
    Process takes the textures by the names of layouts.RECONSTRUCTION_TEXTURES (a missing name is an unbound texture) and the
    Camera.Jitter the frame was rendered with. Runs on the full frame of an unsharded context. No scene is needed."""
    _DTYPE, _RECORD, _LAYOUT = L.RECONSTRUCTION_SETTINGS, "PtReconstructionSettings", "reconstruction_settings"
    _SET, _RESET = "pt_reconstruction_set_constants", "pt_reconstruction_reset_history"

    @property
    def settings(self):
        """the PtReconstructionSettings record last accepted, or None"""
        return self._settings

    def SetConstants(self, settings):
        """settings: PtReconstructionSettings (layouts.reconstruction_settings)."""
        self._set_constants(settings)

    def Process(self, jitter, textures=None):
        tex = self.Textures if textures is None else textures
        t = ReconstructionTextures(*[_ptr(tex.get(n)) for n in L.RECONSTRUCTION_TEXTURES])
        j = (C.c_float * 2)(float(jitter[0]), float(jitter[1]))
        self.ctx.check(self.ctx.lib.pt_reconstruction_process(self.ctx.handle, C.addressof(t), j))

    def DownloadHistory(self):
        """After the last Process: (length, filtered, n). length: the history length of the signal per render pixel, float32 (h, w);
        filtered: what the resolve read, float32 (h, w, 4) (the filtered signal and its variance; the guarded Radiance and 0 where the
        G-buffer missed); n: the accumulated weight per output pixel, float32 (oh, ow). Empty arrays when there is no history.
        Synchronises."""
        render, output = (C.c_uint32 * 2)(), (C.c_uint32 * 2)()
        call = self.ctx.lib.pt_reconstruction_download_history
        self.ctx.check(call(self.ctx.handle, None, None, 0, None, 0, render, output))
        length, filtered = np.zeros((render[1], render[0]), np.float32), np.zeros((render[1], render[0], 4), np.float32)
        n = np.zeros((output[1], output[0]), np.float32)
        if length.size:
            self.ctx.check(call(self.ctx.handle, C.c_void_p(length.ctypes.data), C.c_void_p(filtered.ctypes.data), length.size,
                                C.c_void_p(n.ctypes.data), n.size, render, output))
        return length, filtered, n


class FrameGeneration(_Filter):
    """The library's own frame interpolator for the frame-generation slot of App::PostProcessGraphics (pt_frame_generation_*; DESIGN.md
    section 1, "Frame generation"), where the reference's default settings call DLSS-G after the tone-mapped copy. Not a port of DLSS-G or
    FSR 3, and unpinned against both. From the tone-mapped Color of this frame and of the one before it, with this frame's LinearDepth and
    MotionVector, to the frame at Phase between them. Process takes the textures by the names of layouts.FRAME_GENERATION_TEXTURES (a
    missing name is an unbound texture; Generated8 is optional) and the Camera.Jitter the frame was rendered with. Runs on the full frame
    of an unsharded context. No scene is needed."""
    _DTYPE, _RECORD, _LAYOUT = L.FRAME_GENERATION_SETTINGS, "PtFrameGenerationSettings", "frame_generation_settings"
    _SET, _RESET = "pt_frame_generation_set_constants", "pt_frame_generation_reset_history"

    @property
    def settings(self):
        """the PtFrameGenerationSettings record last accepted, or None"""
        return self._settings

    def SetConstants(self, settings):
        """settings: PtFrameGenerationSettings (layouts.frame_generation_settings)."""
        self._set_constants(settings)

    def Process(self, jitter, textures=None):
        """True when Generated holds an interpolated frame; False on the call that has no previous frame (Generated is then Color)."""
        tex = self.Textures if textures is None else textures
        t = FrameGenerationTextures(*[_ptr(tex.get(n)) for n in L.FRAME_GENERATION_TEXTURES])
        j = (C.c_float * 2)(float(jitter[0]), float(jitter[1]))
        generated = C.c_uint32(0xFFFFFFFF)
        self.ctx.check(self.ctx.lib.pt_frame_generation_process(self.ctx.handle, C.addressof(t), j, C.byref(generated)))
        return bool(generated.value)

    def DownloadField(self):
        """After the last Process that generated a frame: (field, classes). field: the midpoint field, uint64 (h, w) at RenderSize
        (depth bits << 32 | index of the render pixel that won the cell; layouts.FRAME_GENERATION_EMPTY: none); classes: one
        layouts.FRAME_GENERATION_* byte per output pixel, uint8 (oh, ow). Empty arrays when the last call generated nothing. Synchronises."""
        render, output = (C.c_uint32 * 2)(), (C.c_uint32 * 2)()
        call = self.ctx.lib.pt_frame_generation_download_field
        self.ctx.check(call(self.ctx.handle, None, 0, None, 0, render, output))
        field, classes = np.zeros((render[1], render[0]), np.uint64), np.zeros((output[1], output[0]), np.uint8)
        if field.size:
            self.ctx.check(call(self.ctx.handle, C.c_void_p(field.ctypes.data), field.size, C.c_void_p(classes.ctypes.data), classes.size,
                                render, output))
        return field, classes


class Sharpening(_Filter):
    """The library's own edge-adaptive sharpening filter for the image-scaling slot of App::PostProcessGraphics (pt_sharpen_*; DESIGN.md
    section 1, "Sharpening"), where the reference runs App::ProcessNIS (NVIDIA Image Scaling in its sharpen mode) between the upscaler and
    Bloom. Not a port of NVIDIA Image Scaling, and unpinned against it. From the linear HDR Color the post chain would read to Sharpened,
    the same format and size: a high-pass across the edges of the 5 x 5's row, column and diagonals, gated by the contrast of the 3 x 3 and
    limited to its range. Process takes the textures by the names of layouts.SHARPEN_TEXTURES (a missing name is an unbound texture). No
    history, no context-owned memory; no scene is needed. Runs on the full frame: a sharded host calls it on the gathered one."""
    _DTYPE, _RECORD, _LAYOUT = L.SHARPEN_SETTINGS, "PtSharpenSettings", "sharpen_settings"
    _SET = "pt_sharpen_set_constants"

    @property
    def settings(self):
        """the PtSharpenSettings record last accepted, or None"""
        return self._settings

    def SetConstants(self, settings):
        """settings: PtSharpenSettings (layouts.sharpen_settings)."""
        self._set_constants(settings)

    def ResetHistory(self):
        """the pass keeps nothing between calls"""

    def Process(self, textures=None):
        tex = self.Textures if textures is None else textures
        t = SharpenTextures(*[_ptr(tex.get(n)) for n in L.SHARPEN_TEXTURES])
        self.ctx.check(self.ctx.lib.pt_sharpen_process(self.ctx.handle, C.addressof(t)))


class SHARC:
    """Mirror of `struct SHARC` (Source/SHARC.ixx) and of the Raytracing::Render overload that takes it: Configure allocates the context's
    cache, SetConstants takes PtSHARCSettings (layouts.sharc_settings), Render runs clear, update, resolve, query and the swap with the
    GraphicsSettings of raytracing.SetConstants. One cache per context, also for a context that views a shared scene."""

    def __init__(self, ctx):
        self.ctx = ctx
        self._settings = None

    def Configure(self, capacity=0):
        """capacity 0 = 1 << 22 entries; a multiple of 32. Empties the cache."""
        self.ctx.check(self.ctx.lib.pt_sharc_configure(self.ctx.handle, capacity))

    def SetConstants(self, settings):
        self._settings = np.array(settings).reshape(())
        self.ctx.check(self.ctx.lib.pt_sharc_set_constants(self.ctx.handle, C.c_void_p(self._settings.ctypes.data)))

    def Render(self, raytracing, topLevelAccelerationStructure=None):
        """raytracing: the Raytracing operator whose GPUBuffers / Textures the frame uses."""
        ctx, lib = self.ctx, self.ctx.lib
        cam = np.array(raytracing.GPUBuffers["Camera"]); sd = np.array(raytracing.GPUBuffers["SceneData"])
        ctx.check(lib.pt_set_camera(ctx.handle, C.c_void_p(cam.ctypes.data)))
        ctx.check(lib.pt_set_scene_data(ctx.handle, C.c_void_p(sd.ctypes.data)))
        t = _pack_textures(raytracing.Textures)
        ctx.check(lib.pt_raytrace_render_sharc(ctx.handle, C.addressof(t)))

    def Reset(self):
        self.ctx.check(self.ctx.lib.pt_sharc_reset(self.ctx.handle))

    def download(self):
        """The live entries of the resolved buffer (numpy layouts.SHARC_ENTRY). Synchronises."""
        n = C.c_uint32(0)
        self.ctx.check(self.ctx.lib.pt_sharc_download(self.ctx.handle, None, 0, C.byref(n)))
        out = np.zeros(n.value, L.SHARC_ENTRY)
        if n.value:
            self.ctx.check(self.ctx.lib.pt_sharc_download(self.ctx.handle, C.c_void_p(out.ctypes.data), n.value, C.byref(n)))
        return out

    def debug_keys(self, positions, normals):
        """(keys uint64, levels uint32, voxel sizes float32) of points with normals, under the context's camera and SceneScale."""
        p = np.ascontiguousarray(positions, np.float32).reshape(-1, 3); nn = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
        n = len(p)
        keys, levels, sizes = np.zeros(n, np.uint64), np.zeros(n, np.uint32), np.zeros(n, np.float32)
        self.ctx.check(self.ctx.lib.pt_sharc_debug_keys(self.ctx.handle, C.c_void_p(p.ctypes.data), C.c_void_p(nn.ctypes.data), n,
                                                         C.c_void_p(keys.ctypes.data), C.c_void_p(levels.ctypes.data), C.c_void_p(sizes.ctypes.data)))
        return keys, levels, sizes

    def debug_query(self, positions, normals, distances, previous_roughness):
        """The query decision against the resolved buffer (numpy layouts.SHARC_QUERY_RESULT)."""
        p = np.ascontiguousarray(positions, np.float32).reshape(-1, 3); nn = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(distances, np.float32).reshape(-1); r = np.ascontiguousarray(previous_roughness, np.float32).reshape(-1)
        out = np.zeros(len(p), L.SHARC_QUERY_RESULT)
        self.ctx.check(self.ctx.lib.pt_sharc_debug_query(self.ctx.handle, C.c_void_p(p.ctypes.data), C.c_void_p(nn.ctypes.data), C.c_void_p(d.ctypes.data),
                                                          C.c_void_p(r.ctypes.data), len(p), C.c_void_p(out.ctypes.data)))
        return out

    def download_update_paths(self):
        """The vertex log of the last update pass rendered with DEBUG_SHARC_LOG_PATHS: (paths, bounces) of layouts.SHARC_PATH_VERTEX."""
        return _download_counted(self.ctx, self.ctx.lib.pt_sharc_download_update_paths, L.SHARC_PATH_VERTEX, counts=2)

    def download_update_scatter(self):
        """The BSDF steps of the same log: (paths, bounces) of layouts.SHARC_PATH_SCATTER."""
        return _download_counted(self.ctx, self.ctx.lib.pt_sharc_download_update_scatter, L.SHARC_PATH_SCATTER, counts=2)


class Renderer:
    """App::RenderScene for this path (Source/App.cpp:1157-1329): G-buffer pass, then the path tracer."""

    def __init__(self, ctx, scene_gpu, width, height, with_f32=False, with_denoiser_outputs=False, di_history=False):
        self.ctx, self.scene, self.width, self.height = ctx, scene_gpu, width, height
        rank, world, band = getattr(ctx, "sharding", (0, 1, 16))
        self.local_rows = local_rows(height, rank, world, band)
        self.textures = alloc_textures(width, self.local_rows, scene_gpu.device, with_f32, with_denoiser_outputs)
        self.di_history, self._rendered, self._di_brdf_set = di_history, False, False
        self.generated = False                                            # render(..., generate=): textures["Generated"] is an interpolated frame
        if di_history:                                                    # App.cpp:629-634: the DI pass's Previous* G-buffer
            for n in L.DI_PREVIOUS_TEXTURES:
                self.textures[n] = self.textures[n[len("Previous"):]].clone()
        self.gbuffer = GBufferGeneration(ctx)
        self.raytracing = Raytracing(ctx)
        self.direct_lighting = DirectLighting(ctx)
        self.post = PostProcessing(ctx)
        self.sharc = SHARC(ctx)
        self.nrd = NRDComposition(ctx)
        self._denoiser = None
        d = scene_gpu.desc
        for op in (self.gbuffer, self.raytracing, self.direct_lighting):
            op.GPUBuffers["Camera"] = d.camera
            op.GPUBuffers["SceneData"] = d.scene_data
            op.Textures = self.textures
        self.constants = np.zeros((), L.GBUFFER_CONSTANTS)
        self.constants["RenderSize"] = (width, height)
        self.constants["Flags"] = L.GBufferFlags.DefaultNoDenoiser        # App.cpp:1224 with Denoiser::None

    @property
    def denoiser(self):
        """The library's denoiser (Denoiser) bound to this renderer's guide textures, with layouts.denoiser_settings' defaults at the
        renderer's size, created at first use: render(..., nrd=layouts.DENOISER_NRD_RELAX, denoise=renderer.denoiser). Other settings:
        renderer.denoiser.SetConstants. Unsharded contexts only: the filter needs the whole frame."""
        if self._denoiser is None:
            if getattr(self.ctx, "sharding", (0, 1, 16))[1] > 1:
                raise PtInvalidArgument("the denoiser needs the whole frame: run Denoiser on the gathered textures of a sharded render")
            d = Denoiser(self.ctx)
            d.Textures = self.textures                                    # Position, LinearDepth, NormalRoughness, MotionVector
            d.SetConstants(L.denoiser_settings(self.width, self.height))
            self._denoiser = d
        return self._denoiser

    def upscaler(self, output_w, output_h, **overrides):
        """A new Upscaler from this renderer's size to output_w x output_h, bound to the renderer's Radiance, LinearDepth and
        MotionVector, with layouts.upscaler_settings' defaults (overrides by field name): render(..., upscale=that). It writes
        textures["Upscaled"]. Unsharded contexts only: the pass needs the whole frame."""
        if getattr(self.ctx, "sharding", (0, 1, 16))[1] > 1:
            raise PtInvalidArgument("the upscaler needs the whole frame: the context is sharded (run Upscaler on the gathered textures)")
        u = Upscaler(self.ctx)
        u.Textures = self.textures
        u.SetConstants(L.upscaler_settings((self.width, self.height), (output_w, output_h), **overrides))
        return u

    def reconstruction(self, output_w, output_h, **overrides):
        """A new Reconstruction from this renderer's size to output_w x output_h, bound to the renderer's textures, with
        layouts.reconstruction_settings' defaults (overrides by field name): render(..., reconstruct=that) with settings["Denoiser"] =
        DENOISER_DLSS_RR. It writes textures["Reconstructed"]. Unsharded contexts only: the pass needs the whole frame."""
        if getattr(self.ctx, "sharding", (0, 1, 16))[1] > 1:
            raise PtInvalidArgument("the reconstruction needs the whole frame: the context is sharded (run Reconstruction on the gathered textures)")
        u = Reconstruction(self.ctx)
        u.Textures = self.textures
        u.SetConstants(L.reconstruction_settings((self.width, self.height), (output_w, output_h), **overrides))
        return u

    def frame_generation(self, output_w, output_h, **overrides):
        """A new FrameGeneration from this renderer's size to output_w x output_h (the size post= runs at), with
        layouts.frame_generation_settings' defaults (overrides by field name): render(..., post=..., generate=that). It writes
        textures["Generated"] and ["Generated8"]. Unsharded contexts only: the pass needs the whole frame."""
        if getattr(self.ctx, "sharding", (0, 1, 16))[1] > 1:
            raise PtInvalidArgument("frame generation needs the whole frame: the context is sharded (run FrameGeneration on the gathered textures)")
        g = FrameGeneration(self.ctx)
        g.Textures = self.textures
        g.SetConstants(L.frame_generation_settings((self.width, self.height), (output_w, output_h), **overrides))
        return g

    def sharpening(self, w, h, **overrides):
        """A new Sharpening at w x h (the size post= runs at: the upscaler's or the reconstruction's OutputSize, else the renderer's), with
        layouts.sharpen_settings' defaults (overrides by field name): render(..., sharpen=that). It writes textures["Sharpened"]."""
        s = Sharpening(self.ctx)
        s.Textures = self.textures
        s.SetConstants(L.sharpen_settings((w, h), **overrides))
        return s

    def render(self, settings, di_samples=0, di_reuse=None, di_light_sampling=None, post=None, sharc=None, di_visibility=None, di_pairwise=None,
               di_regir_layout=None, di_brdf=None, nrd=None, denoise=None, nrd_hit_distance=None, di_pdf_mipmap=None, upscale=None,
               reconstruct=None, generate=None, sharpen=None):
        """sharpen: a Sharpening (self.sharpening(w, h)) to run the image-scaling step of App::PostProcessGraphics (ProcessNIS,
        App.cpp:1544-1548) after upscale= / reconstruct= when given, else after the frame, and before post: it reads the texture post=
        would have read (Upscaled, Reconstructed, else Radiance) and writes textures["Sharpened"], which post=, when given, then reads
        as its Radiance. Its Size must be the size post= runs at. None: no such step, nothing changes.
        generate: a FrameGeneration (self.frame_generation(output_w, output_h)) to run the frame-generation step of
        App::PostProcessGraphics (App.cpp:1564-1566) after the post chain: it reads textures["Color"] (post= is required, at the pass's
        OutputSize), the frame's LinearDepth and MotionVector and the camera's Jitter and writes textures["Generated"] and
        ["Generated8"]; self.generated tells whether that is an interpolated frame (False on the frame without a predecessor: a copy of
        Color). None: no such step, nothing changes.
        reconstruct: a Reconstruction (self.reconstruction(output_w, output_h)) to run the ray-reconstruction step of
        App::PostProcessGraphics (App.cpp:1513-1523) after the frame and before post, where upscale= runs: it reads the frame's noisy
        Radiance, the albedos, the guides and the camera's Jitter and writes textures["Reconstructed"] at its OutputSize; post's
        RenderSize must then be that OutputSize and the post chain reads Reconstructed as its Radiance. settings["Denoiser"] must be
        DENOISER_DLSS_RR (the frame then writes what the pass reads); not together with upscale or nrd (the pass is both steps).
        upscale: an Upscaler (self.upscaler(output_w, output_h)) to run the super-resolution step of App::PostProcessGraphics
        (App.cpp:1532-1541) after the NRD block and before post: it reads the frame's Radiance, LinearDepth and MotionVector and the
        camera's Jitter and writes textures["Upscaled"] at its OutputSize; post's RenderSize must then be that OutputSize and the post
        chain reads Upscaled as its Radiance. None: no such step, the frame as it was.
        di_pdf_mipmap: True / False for DirectLighting.SetPdfMipmap ahead of the DI pass, or None: the context's setting is left alone.
        nrd: layouts.DENOISER_NRD_REBLUR / _RELAX (it must be settings' Denoiser) to run App::ProcessNRD (App.cpp:1595-1688) after the
        frame and before post: the NRD composition pass packs textures["Diffuse"] / ["Specular"] in place, denoise(noisy_diffuse,
        noisy_specular) -> (denoised_diffuse, denoised_specular) takes and returns device tensors of their shape (None: the identity,
        the denoised textures alias the noisy ones; self.denoiser: the library's own filter, ReLAX only), and the pass composes the result
        into textures["Radiance"]. It needs a renderer with
        with_denoiser_outputs=True; the G-buffer call then carries the albedo flags. nrd_hit_distance: the four ReBLUR hit-distance
        parameters, None: the defaults. Works on a sharded context (on its own rows).
        di_brdf: layouts.di_brdf_settings for BRDF candidates in the DI pass's initial sampling, or None: none (the
        setter is then called only to turn off what an earlier frame of this renderer turned on).
        di_samples > 0: run the DI pass with that many candidates per pixel; set settings["IsDIEnabled"] to have the path tracer
        consume it (the textures need Diffuse / Specular: with_denoiser_outputs=True). di_reuse: PtDIResamplingSettings
        (layouts.di_resampling_settings) for reservoir reuse; temporal reuse needs di_history=True. With di_history the current and
        Previous* G-buffer textures are swapped before each frame after the first, so that after render() the current ones hold this
        frame's G-buffer and the Previous* ones the last frame's. di_light_sampling: PtDILightSamplingSettings
        (layouts.di_light_sampling_settings), or None: the power CDF. di_visibility: PtDIVisibilitySettings (layouts.di_visibility_settings)
        for visibility in the reservoirs (initial visibility, Raytraced bias correction, final-visibility reuse), or None: none. di_pairwise: PtDIPairwiseSettings
        (layouts.di_pairwise_settings) to turn a pass's Basic bias correction into Pairwise, or None: off. di_regir_layout: PtDIReGIRLayoutSettings
        (layouts.di_regir_layout_settings) for the layout of the ReGIR cells, or None: the Grid. post: PtPostProcessSettings (layouts.post_processing_settings) to run
        the post-processing chain on the frame's Radiance; it writes textures["Color"], ["BackBuffer"] and ["Display8"]. Unsharded
        contexts only: a sharded host gathers Radiance and runs PostProcessing on the full frame. sharc: PtSHARCSettings
        (layouts.sharc_settings) to render the frame through the radiance cache (self.sharc.Configure first); None: the plain path tracer."""
        tlas = self.scene.GetTopLevelAccelerationStructure()
        if post is not None:
            p = np.array(post).reshape(())
            if getattr(self.ctx, "sharding", (0, 1, 16))[1] > 1:
                raise PtInvalidArgument("post-processing needs the whole frame: run PostProcessing on the gathered Radiance of a sharded render")
            if upscale is None and reconstruct is None and tuple(int(v) for v in p["RenderSize"]) != (self.width, self.height):
                raise PtInvalidArgument("post-processing RenderSize differs from the renderer's size")
        out_w = out_h = None
        if reconstruct is not None:
            if not isinstance(reconstruct, Reconstruction) or reconstruct.settings is None:
                raise PtInvalidArgument("reconstruct must be a Reconstruction whose constants are set (Renderer.reconstruction)")
            if upscale is not None or nrd is not None:
                raise PtInvalidArgument("reconstruct cannot be combined with upscale or nrd: ray reconstruction is the denoiser and the upscaler of its frame")
            if int(np.array(settings).reshape(())["Denoiser"]) != L.DENOISER_DLSS_RR:
                raise PtInvalidArgument("reconstruct needs settings['Denoiser'] = DENOISER_DLSS_RR: only then the frame writes the noisy Radiance and the albedos the pass reads")
            if "DiffuseAlbedo" not in self.textures or "SpecularAlbedo" not in self.textures:
                raise PtInvalidArgument("reconstruct needs the DiffuseAlbedo / SpecularAlbedo textures: the renderer has none")
            if getattr(self.ctx, "sharding", (0, 1, 16))[1] > 1:
                raise PtInvalidArgument("the reconstruction needs the whole frame: the context is sharded")
            if tuple(int(v) for v in reconstruct.settings["RenderSize"]) != (self.width, self.height):
                raise PtInvalidArgument("the reconstruction's RenderSize differs from the renderer's size")
            out_w, out_h = (int(v) for v in reconstruct.settings["OutputSize"])
            if post is not None and tuple(int(v) for v in p["RenderSize"]) != (out_w, out_h):
                raise PtInvalidArgument("post-processing RenderSize differs from the reconstruction's OutputSize")
        if upscale is not None:
            if not isinstance(upscale, Upscaler) or upscale.settings is None:
                raise PtInvalidArgument("upscale must be an Upscaler whose constants are set (Renderer.upscaler)")
            if getattr(self.ctx, "sharding", (0, 1, 16))[1] > 1:
                raise PtInvalidArgument("the upscaler needs the whole frame: the context is sharded")
            if tuple(int(v) for v in upscale.settings["RenderSize"]) != (self.width, self.height):
                raise PtInvalidArgument("the upscaler's RenderSize differs from the renderer's size")
            out_w, out_h = (int(v) for v in upscale.settings["OutputSize"])
            if post is not None and tuple(int(v) for v in p["RenderSize"]) != (out_w, out_h):
                raise PtInvalidArgument("post-processing RenderSize differs from the upscaler's OutputSize")
        if generate is not None:
            if post is None:
                raise PtInvalidArgument("generate needs post: the pass interpolates the tone-mapped Color the post chain writes")
            if not isinstance(generate, FrameGeneration) or generate.settings is None:
                raise PtInvalidArgument("generate must be a FrameGeneration whose constants are set (Renderer.frame_generation)")
            if tuple(int(v) for v in generate.settings["RenderSize"]) != (self.width, self.height):
                raise PtInvalidArgument("the frame generation's RenderSize differs from the renderer's size")
            if tuple(int(v) for v in generate.settings["OutputSize"]) != tuple(int(v) for v in p["RenderSize"]):
                raise PtInvalidArgument("the frame generation's OutputSize differs from the post-processing RenderSize")
        if sharpen is not None:
            if not isinstance(sharpen, Sharpening) or sharpen.settings is None:
                raise PtInvalidArgument("sharpen must be a Sharpening whose constants are set (Renderer.sharpening)")
            if getattr(self.ctx, "sharding", (0, 1, 16))[1] > 1:
                raise PtInvalidArgument("sharpening needs the whole frame: the context is sharded (run Sharpening on the gathered frame)")
            if tuple(int(v) for v in sharpen.settings["Size"]) != ((self.width, self.height) if out_w is None else (out_w, out_h)):
                raise PtInvalidArgument("the sharpening's Size differs from the size the post chain runs at")
        if self.di_history and self._rendered:
            for n in L.DI_PREVIOUS_TEXTURES:
                c = n[len("Previous"):]
                self.textures[n], self.textures[c] = self.textures[c], self.textures[n]
        denoiser = int(np.array(settings).reshape(())["Denoiser"])
        if nrd is None and denoise is not None:
            raise PtInvalidArgument("denoise is given without nrd: name the NRD denoiser value whose packing it reads")
        if nrd is not None:
            if int(nrd) not in (L.DENOISER_NRD_REBLUR, L.DENOISER_NRD_RELAX):
                raise PtInvalidArgument("nrd must be DENOISER_NRD_REBLUR or DENOISER_NRD_RELAX")
            if denoiser != int(nrd):
                raise PtInvalidArgument("nrd differs from the settings' Denoiser: the frame must write the NRD-facing outputs the pass packs")
            if isinstance(denoise, Denoiser) and int(nrd) != L.DENOISER_NRD_RELAX:
                raise PtInvalidArgument("the library's Denoiser reads ReLAX's packing only: ReBLUR's (YCoCg, normalised hit distance) is not served")
            if "Diffuse" not in self.textures or "Specular" not in self.textures:
                raise PtInvalidArgument("nrd needs the Diffuse / Specular textures: create the Renderer with with_denoiser_outputs=True")
            nrd_pack = L.nrd_composition_constants(self.width, self.local_rows, int(nrd), True, nrd_hit_distance)
            nrd_compose = L.nrd_composition_constants(self.width, self.local_rows, int(nrd), False, nrd_hit_distance)
        self.constants["Flags"] = 0xFFFFFFFF if denoiser != L.DENOISER_NONE else L.GBufferFlags.DefaultNoDenoiser   # App.cpp:1223
        if nrd is not None and int(self.constants["Flags"]) & L.GBufferFlags.Albedo != L.GBufferFlags.Albedo:
            raise PtInvalidArgument("nrd needs DiffuseAlbedo / SpecularAlbedo: the G-buffer call lacks the albedo flags")
        self.gbuffer.Render(tlas, self.constants)
        if di_samples:                                                    # App.cpp:1234-1308: the DI pass between the two
            s = np.array(settings).reshape(())
            self.direct_lighting.SetConstants(L.di_settings(self.width, self.height, int(s["FrameIndex"]), di_samples, denoiser,
                                                            last_pass=int(s["Bounces"]) == 0, ext_flags=int(s["ExtFlags"])))
            self.direct_lighting.SetResampling(di_reuse)
            self.direct_lighting.SetLightSampling(di_light_sampling)
            self.direct_lighting.SetVisibility(di_visibility)
            self.direct_lighting.SetPairwise(di_pairwise)
            self.direct_lighting.SetReGIRLayout(di_regir_layout)
            if di_brdf is not None or self._di_brdf_set:
                self.direct_lighting.SetBrdfSampling(di_brdf)
                self._di_brdf_set = di_brdf is not None
            if di_pdf_mipmap is not None:
                self.direct_lighting.SetPdfMipmap(di_pdf_mipmap)
            self.direct_lighting.Render(tlas)
        if int(np.array(settings).reshape(())["Bounces"]) > 0:            # App.cpp:1277
            self.raytracing.SetConstants(settings)
            if sharc is not None:                                         # the Render overload with RTXGITechnique::SHARC
                self.sharc.SetConstants(sharc)
                self.sharc.Render(self.raytracing, tlas)
            else:
                self.raytracing.Render(tlas)
        if nrd is not None:                                               # App::ProcessNRD, App.cpp:1595-1688: pack, the denoiser, compose
            t = self.textures
            tex = {n: t[n] for n in ("LinearDepth", "DiffuseAlbedo", "SpecularAlbedo", "NormalRoughness", "Radiance")}
            tex["NoisyDiffuse"], tex["NoisySpecular"] = t["Diffuse"], t["Specular"]
            self.nrd.Process(tex, nrd_pack)
            dd, ds = (t["Diffuse"], t["Specular"]) if denoise is None else denoise(t["Diffuse"], t["Specular"])
            for name, got, like in (("diffuse", dd, t["Diffuse"]), ("specular", ds, t["Specular"])):
                if got is None or got.dtype != like.dtype or tuple(got.shape) != tuple(like.shape) or got.device != like.device or not got.is_contiguous():
                    raise PtInvalidArgument(f"denoise returned a {name} texture that is not a contiguous device tensor of the noisy one's shape and dtype")
            tex["DenoisedDiffuse"], tex["DenoisedSpecular"] = dd, ds
            self.nrd.Process(tex, nrd_compose)
            self._nrd_keep = (dd, ds)                                     # the compose is enqueued: its inputs live until the next frame
        if upscale is not None:                                           # App.cpp:1532-1541: between the denoiser and Bloom / ToneMap
            t = self.textures
            if "Upscaled" not in t or tuple(t["Upscaled"].shape) != (out_h, out_w, 4):
                t["Upscaled"] = _torch().zeros((out_h, out_w, 4), dtype=t["Radiance"].dtype, device=self.scene.device)
            jitter = np.array(self.gbuffer.GPUBuffers["Camera"]).reshape(())["Jitter"]
            # the context's settings are this upscaler's (the same again keep the history): they size what the call writes
            upscale.SetConstants(upscale.settings)
            upscale.Process(jitter, {"Radiance": t["Radiance"], "LinearDepth": t["LinearDepth"], "MotionVector": t["MotionVector"],
                                     "Color": t["Upscaled"]})
        if reconstruct is not None:                                       # App.cpp:1513-1523: ProcessDLSSRayReconstruction's place
            t = self.textures
            if "Reconstructed" not in t or tuple(t["Reconstructed"].shape) != (out_h, out_w, 4):
                t["Reconstructed"] = _torch().zeros((out_h, out_w, 4), dtype=t["Radiance"].dtype, device=self.scene.device)
            jitter = np.array(self.gbuffer.GPUBuffers["Camera"]).reshape(())["Jitter"]
            # the context's settings are this pass's (the same again keep the history): they size what the call writes
            reconstruct.SetConstants(reconstruct.settings)
            reconstruct.Process(jitter, dict({n: t[n] for n in L.RECONSTRUCTION_TEXTURES[:-1]}, Color=t["Reconstructed"]))
        if sharpen is not None:                                           # App.cpp:1544-1548: ProcessNIS, between the upscaler and Bloom
            t = self.textures
            source = "Upscaled" if upscale is not None else "Reconstructed" if reconstruct is not None else "Radiance"
            if "Sharpened" not in t or tuple(t["Sharpened"].shape) != tuple(t[source].shape):
                t["Sharpened"] = _torch().zeros(tuple(t[source].shape), dtype=t[source].dtype, device=self.scene.device)
            sharpen.SetConstants(sharpen.settings)                        # the context's settings are this pass's
            sharpen.Process({"Color": t[source], "Sharpened": t["Sharpened"]})
        if post is not None:                                              # App.cpp:1506-1571, after Raytracing::Render
            pw, ph = (out_w, out_h) if upscale is not None or reconstruct is not None else (self.width, self.height)
            if "Color" not in self.textures or tuple(self.textures["Color"].shape[:2]) != (ph, pw):
                self.textures.update(alloc_post_textures(pw, ph, self.scene.device))
            self.post.SetConstants(post)
            resized = "Sharpened" if sharpen is not None else "Upscaled" if upscale is not None else "Reconstructed" if reconstruct is not None else None
            self.post.Render(self.textures if resized is None else dict(self.textures, Radiance=self.textures[resized]))
        if generate is not None:                                          # App.cpp:1564-1566: behind ToneMap, where DLSS-G is tagged
            t = self.textures
            gw, gh = (int(v) for v in generate.settings["OutputSize"])
            if "Generated" not in t or tuple(t["Generated"].shape) != (gh, gw, 4):
                t["Generated"] = _torch().zeros((gh, gw, 4), dtype=t["Color"].dtype, device=self.scene.device)
                t["Generated8"] = _torch().zeros((gh, gw, 4), dtype=_torch().uint8, device=self.scene.device)   # like Display8: four bytes a pixel
            jitter = np.array(self.gbuffer.GPUBuffers["Camera"]).reshape(())["Jitter"]
            # the context's settings are this pass's (the same again keep the previous frame)
            generate.SetConstants(generate.settings)
            self.generated = generate.Process(jitter, {n: t[n] for n in L.FRAME_GENERATION_TEXTURES})
        self._rendered = True
