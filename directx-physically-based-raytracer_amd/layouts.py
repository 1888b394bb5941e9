"""Byte-exact numpy mirrors of the reference's GPU data layouts.

Reference: Source/CommonShaderData.ixx:15-39 (SceneData, InstanceData, MeshDescriptors, ObjectData),
Source/Material.ixx:10-38, Source/Vertex.ixx:30-50, Source/Camera.ixx:16-36,
Source/Raytracing.ixx:151-166 (GraphicsSettings), Source/GBufferGeneration.ixx:28-49.
The C side of the same layouts is include/ptamd.h (static_asserted there).
"""
import numpy as np

NONE = 0xFFFFFFFF  # "~0u": absent attribute / descriptor

VERTEX = np.dtype({  # VertexPositionNormalTangentTexture, 32 B
    "names": ["Position", "Normal", "Tangent", "TexCoord0", "TexCoord1"],
    "formats": [("<f4", 3), ("<i2", 3), ("<i2", 3), ("<f2", 2), ("<f2", 2)],
    "offsets": [0, 12, 18, 24, 28], "itemsize": 32})

SKELETAL_VERTEX = np.dtype({  # VertexPositionNormalTangentSkin, 48 B (Source/Vertex.ixx:52-57)
    "names": ["Position", "Normal", "Tangent", "Joints", "Weights"],
    "formats": [("<f4", 3), ("<i2", 3), ("<i2", 3), ("<u2", 4), ("<f4", 4)],
    "offsets": [0, 12, 18, 24, 32], "itemsize": 48})

VERTEX_DESC = np.dtype({
    "names": ["Stride", "Normal", "Tangent", "TexCoord"],
    "formats": ["<u4", "<u4", "<u4", ("<u4", 2)],
    "offsets": [0, 16, 20, 24], "itemsize": 32})

MESH_DESCRIPTORS = np.dtype({
    "names": ["Vertices", "Indices", "MotionVectors"],
    "formats": ["<u4", "<u4", "<u4"], "offsets": [0, 4, 8], "itemsize": 16})

MATERIAL = np.dtype({
    "names": ["BaseColor", "EmissiveStrength", "EmissiveColor", "Metallic", "Roughness", "IOR",
              "Transmission", "AlphaMode", "AlphaCutoff"],
    "formats": [("<f4", 4), "<f4", ("<f4", 3), "<f4", "<f4", "<f4", "<f4", "<u4", "<f4"],
    "offsets": [0, 16, 20, 32, 36, 40, 44, 48, 52], "itemsize": 64})

TEXTURE_MAP_INFO = np.dtype({
    "names": ["Descriptor", "TextureCoordinateIndex"], "formats": ["<u4", "<u4"],
    "offsets": [0, 4], "itemsize": 16})

OBJECT_DATA = np.dtype({
    "names": ["VertexDesc", "MeshDescriptors", "Material", "TextureMapInfoArray"],
    "formats": [VERTEX_DESC, MESH_DESCRIPTORS, MATERIAL, (TEXTURE_MAP_INFO, 7)],
    "offsets": [0, 32, 48, 112], "itemsize": 224})

INSTANCE_DATA = np.dtype({
    "names": ["FirstGeometryIndex", "PreviousObjectToWorld", "ObjectToWorld"],
    "formats": ["<u4", ("<f4", (3, 4)), ("<f4", (3, 4))],
    "offsets": [0, 16, 64], "itemsize": 112})

SCENE_DATA = np.dtype({
    "names": ["IsStatic", "IsEnvironmentLightTextureCubeMap", "EnvironmentLightTextureDescriptor",
              "EnvironmentLightColor", "EnvironmentLightTransform"],
    "formats": ["<u4", "<u4", "<u4", ("<f4", 4), ("<f4", (3, 4))],
    "offsets": [0, 4, 8, 16, 32], "itemsize": 80})

_M = ("<f4", (4, 4))
CAMERA = np.dtype({
    "names": ["IsNormalizedDepthReversed", "PreviousPosition", "Position", "RightDirection",
              "UpDirection", "ForwardDirection", "ApertureRadius", "NearDepth", "FarDepth", "Jitter",
              "PreviousWorldToView", "PreviousViewToProjection", "PreviousWorldToProjection",
              "PreviousProjectionToView", "PreviousViewToWorld", "WorldToProjection",
              "ProjectionToView", "ViewToWorld"],
    "formats": ["<u4", ("<f4", 3), ("<f4", 3), ("<f4", 3), ("<f4", 3), ("<f4", 3), "<f4", "<f4", "<f4",
                ("<f4", 2), _M, _M, _M, _M, _M, _M, _M, _M],
    "offsets": [0, 4, 16, 32, 48, 64, 76, 80, 84, 88, 96, 160, 224, 288, 352, 416, 480, 544],
    "itemsize": 608})

GRAPHICS_SETTINGS = np.dtype({
    "names": ["RenderSize", "FrameIndex", "Bounces", "SamplesPerPixel", "ThroughputThreshold",
              "IsRussianRouletteEnabled", "IsShaderExecutionReorderingEnabled", "IsDIEnabled", "Denoiser",
              "ExtFlags"],
    "formats": [("<u4", 2), "<u4", "<u4", "<u4", "<f4", "<u4", "<u4", "<u4", "<u4", "<u4"],
    "offsets": [0, 8, 12, 16, 20, 24, 28, 32, 36, 40], "itemsize": 80})

EXT_LAMBERTIAN_ONLY = 0x1   # build-side switch living in the reference's padding word (config C1)

DI_SETTINGS = np.dtype({  # PtDISettings (include/ptamd.h): RTXDI::SetConstants of this library's DI pass
    "names": ["RenderSize", "FrameIndex", "LocalLightSamples", "Denoiser", "IsLastRenderPass", "ExtFlags"],
    "formats": [("<u4", 2), "<u4", "<u4", "<u4", "<u4", "<u4"],
    "offsets": [0, 8, 12, 16, 20, 24], "itemsize": 32})

TRIANGLE_LIGHT = np.dtype({  # PtTriangleLight: one emissive triangle, world space (TriangleLight::Initialize, Light.hlsli)
    "names": ["Base", "Area", "Edge0", "Power", "Edge1", "InstanceIndex", "Normal", "PrimitiveIndex", "Radiance", "GeometryIndex"],
    "formats": [("<f4", 3), "<f4", ("<f4", 3), "<f4", ("<f4", 3), "<u4", ("<f4", 3), "<u4", ("<f4", 3), "<u4"],
    "offsets": [0, 12, 16, 28, 32, 44, 48, 60, 64, 76], "itemsize": 80})


def di_settings(width, height, frame_index=0, samples=8, denoiser=0, last_pass=False, ext_flags=0):
    """PtDISettings with the reference's defaults (LocalLightSamples 8)."""
    s = np.zeros((), DI_SETTINGS)
    s["RenderSize"] = (width, height)
    s["FrameIndex"] = frame_index
    s["LocalLightSamples"] = samples
    s["Denoiser"] = denoiser
    s["IsLastRenderPass"] = 1 if last_pass else 0
    s["ExtFlags"] = ext_flags
    return s

DI_BIAS_CORRECTION_OFF, DI_BIAS_CORRECTION_BASIC = 0, 1

DI_RESAMPLING_SETTINGS = np.dtype({  # PtDIResamplingSettings: ReSTIRDI.TemporalResampling / SpatialResampling (Source/MyAppData.h:226-247)
    "names": ["TemporalResampling", "TemporalBiasCorrection", "MaxHistoryLength", "BoilingFilter", "BoilingFilterStrength",
              "TemporalDepthThreshold", "TemporalNormalThreshold", "SpatialSamples", "SpatialBiasCorrection", "DisocclusionBoostSamples",
              "SpatialSamplingRadius", "SpatialDepthThreshold", "SpatialNormalThreshold"],
    "formats": ["<u4", "<u4", "<u4", "<u4", "<f4", "<f4", "<f4", "<u4", "<u4", "<u4", "<f4", "<f4", "<f4"],
    "offsets": [0, 4, 8, 12, 16, 20, 24, 28, 32, 36, 40, 44, 48], "itemsize": 64})

DI_RESERVOIR = np.dtype({  # PtDIReservoir: one per pixel, row-major; Visibility: di_unpack_visibility (0 unless di_visibility is on)
    "names": ["LightIndex", "U", "V", "W", "M", "TargetPdf", "Age", "Visibility"],
    "formats": ["<u4", "<f4", "<f4", "<f4", "<u4", "<f4", "<u4", "<u4"],
    "offsets": [0, 4, 8, 12, 16, 20, 24, 28], "itemsize": 32})

PT_DI_VISIBILITY_SETTINGS = np.dtype({  # PtDIVisibilitySettings: visibility in the reservoirs (pt_di_set_visibility)
    "names": ["InitialVisibility", "FinalVisibilityReuse", "FinalVisibilityMaxAge", "FinalVisibilityMaxDistance", "DiscardInvisibleSamples",
              "TemporalRaytraced", "SpatialRaytraced"],
    "formats": ["<u4", "<u4", "<u4", "<f4", "<u4", "<u4", "<u4"], "offsets": [0, 4, 8, 12, 16, 20, 24], "itemsize": 32})


def di_visibility_settings(initial=True, final_reuse=True, max_age=4, max_distance=16.0, discard_invisible=False,
                           temporal_raytraced=False, spatial_raytraced=False):
    """PtDIVisibilitySettings. The defaults are the RTXDI SDK's from memory (not in the reference tree, unpinned): initial visibility and
    final-visibility reuse on, 4 frames, 16 pixels, invisible samples kept. *_raytraced turn a pass's Basic normalisation into Raytraced."""
    s = np.zeros((), PT_DI_VISIBILITY_SETTINGS)
    s["InitialVisibility"] = 1 if initial else 0
    s["FinalVisibilityReuse"] = 1 if final_reuse else 0
    s["FinalVisibilityMaxAge"] = max_age
    s["FinalVisibilityMaxDistance"] = max_distance
    s["DiscardInvisibleSamples"] = 1 if discard_invisible else 0
    s["TemporalRaytraced"] = 1 if temporal_raytraced else 0
    s["SpatialRaytraced"] = 1 if spatial_raytraced else 0
    return s


PT_DI_PAIRWISE_SETTINGS = np.dtype({  # PtDIPairwiseSettings: pairwise-MIS bias correction of the reuse passes (pt_di_set_pairwise)
    "names": ["TemporalPairwise", "SpatialPairwise", "Reserved"], "formats": ["<u4", "<u4", ("<u4", 2)], "offsets": [0, 4, 8], "itemsize": 16})


def di_pairwise_settings(temporal=False, spatial=False):
    """PtDIPairwiseSettings: a flag turns the Basic normalisation of its pass (di_resampling_settings' *_bias = DI_BIAS_CORRECTION_BASIC)
    into ReSTIRDI's Pairwise bias correction. Both off by default."""
    s = np.zeros((), PT_DI_PAIRWISE_SETTINGS)
    s["TemporalPairwise"] = 1 if temporal else 0
    s["SpatialPairwise"] = 1 if spatial else 0
    return s


def di_unpack_visibility(word):
    """PtDIReservoir.Visibility (array or scalar) -> (rgb visibility [..., 3] in [0, 1], dx, dy, age): 5 bits per channel decoded / 31,
    two 6-bit two's-complement pixel offsets, a 4-bit age."""
    w = np.asarray(word, np.uint32).astype(np.int64)
    rgb = np.stack([w & 31, (w >> 5) & 31, (w >> 10) & 31], -1) / 31.0
    dx, dy = (w >> 15) & 63, (w >> 21) & 63
    return rgb, dx - 2 * (dx & 32), dy - 2 * (dy & 32), (w >> 27) & 15


def di_pack_visibility(rgb, dx=0, dy=0, age=0):
    """the inverse of di_unpack_visibility, with the device's clamps: uint(clamp(v, 0, 1) * 31) in float32, d to +-31, age to 15"""
    c = (np.clip(np.asarray(rgb, np.float32), np.float32(0), np.float32(1)) * np.float32(31)).astype(np.uint32)
    dx, dy = int(np.clip(dx, -31, 31)) & 63, int(np.clip(dy, -31, 31)) & 63
    return int(c[0]) | int(c[1]) << 5 | int(c[2]) << 10 | dx << 15 | dy << 21 | min(int(age), 15) << 27

DI_LOCAL_LIGHT_POWER_CDF, DI_LOCAL_LIGHT_UNIFORM, DI_LOCAL_LIGHT_POWER_RIS, DI_LOCAL_LIGHT_REGIR_RIS = 0, 1, 2, 3
DI_LOCAL_LIGHT_MODES = {"cdf": DI_LOCAL_LIGHT_POWER_CDF, "uniform": DI_LOCAL_LIGHT_UNIFORM, "power_ris": DI_LOCAL_LIGHT_POWER_RIS,
                        "regir": DI_LOCAL_LIGHT_REGIR_RIS}

DI_LIGHT_SAMPLING_SETTINGS = np.dtype({  # PtDILightSamplingSettings: ReSTIRDI.InitialSampling.LocalLight.Mode, ReGIR.{Cell.Size, BuildSamples}
    "names": ["Mode", "ReGIRCellSize", "ReGIRBuildSamples"], "formats": ["<u4", "<f4", "<u4"], "offsets": [0, 4, 8], "itemsize": 16})

DI_PRESAMPLED_LIGHT = np.dtype({  # PtDIPresampledLight: a Power_RIS tile entry or a ReGIR cell slot; LightIndex 0xFFFFFFFF = empty
    "names": ["LightIndex", "InvSourcePdf"], "formats": ["<u4", "<f4"], "offsets": [0, 4], "itemsize": 8})


def di_light_sampling_settings(mode="regir", cell_size=1.0, build_samples=8):
    """PtDILightSamplingSettings with the reference's defaults (Source/MyAppData.h:200-215): ReGIR_RIS, cell size 1, 8 build samples.
    mode: "cdf" (this library's default), "uniform", "power_ris", "regir", or a DI_LOCAL_LIGHT_* value."""
    s = np.zeros((), DI_LIGHT_SAMPLING_SETTINGS)
    s["Mode"] = DI_LOCAL_LIGHT_MODES[mode] if isinstance(mode, str) else mode
    s["ReGIRCellSize"] = cell_size
    s["ReGIRBuildSamples"] = build_samples
    return s


DI_REGIR_LAYOUT_GRID, DI_REGIR_LAYOUT_ONION = 0, 1
DI_REGIR_LAYOUTS = {"grid": DI_REGIR_LAYOUT_GRID, "onion": DI_REGIR_LAYOUT_ONION}

DI_REGIR_LAYOUT_SETTINGS = np.dtype({  # PtDIReGIRLayoutSettings: the layout of the ReGIR cells (pt_di_set_regir_layout)
    "names": ["Layout", "_pad"], "formats": ["<u4", ("<u4", 3)], "offsets": [0, 4], "itemsize": 16})


def di_regir_layout_settings(layout="grid"):
    """PtDIReGIRLayoutSettings. layout: "grid" (this library's default: 16 x 16 x 16 cubes), "onion" (the reference's compiled
    RTXDI_REGIR_ONION: 2253 cells in concentric shells around the camera), or a DI_REGIR_LAYOUT_* value. It acts only in ReGIR mode."""
    s = np.zeros((), DI_REGIR_LAYOUT_SETTINGS)
    s["Layout"] = DI_REGIR_LAYOUTS[layout] if isinstance(layout, str) else layout
    return s


DI_BRDF_SETTINGS = np.dtype({  # the arguments of pt_di_set_brdf_sampling (BRDF candidates of initial sampling) as one record
    "names": ["BrdfSamples", "BrdfCutoff", "_pad"], "formats": ["<u4", "<f4", ("<u4", 2)], "offsets": [0, 4, 8], "itemsize": 16})

DI_BRDF_CANDIDATE = np.dtype({  # the four words of a record of pt_di_download_brdf_candidates: one per pixel and BRDF candidate, pixel-major; LightIndex 0xFFFFFFFF = no light at the end of the ray
    "names": ["LightIndex", "U", "V", "BrdfPdf"], "formats": ["<u4", "<f4", "<f4", "<f4"], "offsets": [0, 4, 8, 12], "itemsize": 16})


def di_brdf_settings(samples=1, cutoff=0.0):
    """pt_di_set_brdf_sampling's arguments with the reference's default (Source/MyAppData.h:220-221): BRDFSamples 1. cutoff in [0, 1): a BRDF ray ends at
    sqrt((1 / cutoff - 1) * pdf); 0, this library's default, leaves the rays unbounded. The RTXDI SDK's own cutoff default is 1e-4 from
    memory (the SDK is not in the reference tree, unpinned)."""
    s = np.zeros((), DI_BRDF_SETTINGS)
    s["BrdfSamples"] = samples
    s["BrdfCutoff"] = cutoff
    return s


DI_PREVIOUS_TEXTURES = ["PreviousGeometricNormal", "PreviousLinearDepth", "PreviousBaseColorMetalness", "PreviousNormalRoughness",
                        "PreviousIOR", "PreviousTransmission"]   # PtDIPreviousTextures member order


def di_resampling_settings(temporal=True, spatial_samples=1, temporal_bias=DI_BIAS_CORRECTION_BASIC, spatial_bias=DI_BIAS_CORRECTION_BASIC,
                           boiling_filter=True, boiling_strength=0.2, max_history=20, temporal_depth=0.1, temporal_normal=0.5,
                           boost_samples=8, radius=32.0, spatial_depth=0.1, spatial_normal=0.5):
    """PtDIResamplingSettings. From the reference (MyAppData.h): Basic bias correction for both passes, the boiling filter on at 0.2,
    1 spatial sample. From the RTXDI SDK's documented defaults (not in the reference tree): max history 20, depth / normal thresholds
    0.1 / 0.5, spatial radius 32 px, 8 disocclusion-boost samples."""
    s = np.zeros((), DI_RESAMPLING_SETTINGS)
    s["TemporalResampling"] = 1 if temporal else 0
    s["TemporalBiasCorrection"] = temporal_bias
    s["MaxHistoryLength"] = max_history
    s["BoilingFilter"] = 1 if boiling_filter else 0
    s["BoilingFilterStrength"] = boiling_strength
    s["TemporalDepthThreshold"] = temporal_depth
    s["TemporalNormalThreshold"] = temporal_normal
    s["SpatialSamples"] = spatial_samples
    s["SpatialBiasCorrection"] = spatial_bias
    s["DisocclusionBoostSamples"] = boost_samples
    s["SpatialSamplingRadius"] = radius
    s["SpatialDepthThreshold"] = spatial_depth
    s["SpatialNormalThreshold"] = spatial_normal
    return s


POST_PROCESS_SETTINGS = np.dtype({  # PtPostProcessSettings: PostProcessing.{Bloom, ToneMapping} (Source/MyAppData.h:305-333)
    "names": ["RenderSize", "IsBloomEnabled", "BloomStrength", "IsHDREnabled", "ToneMappingOperator", "Exposure", "PaperWhiteNits",
              "ColorPrimaryRotation"],
    "formats": [("<u4", 2), "<u4", "<f4", "<u4", "<u4", "<f4", "<f4", "<u4"],
    "offsets": [0, 8, 12, 16, 20, 24, 28, 32], "itemsize": 48})

TONE_MAP_SATURATE, TONE_MAP_REINHARD, TONE_MAP_ACES_FILMIC = 1, 2, 3          # ToneMapPostProcess::Operator
TONE_MAP_OPERATORS = {"saturate": TONE_MAP_SATURATE, "reinhard": TONE_MAP_REINHARD, "aces_filmic": TONE_MAP_ACES_FILMIC}
COLOR_ROTATION_HDTV_TO_UHDTV, COLOR_ROTATION_DCI_P3_D65_TO_UHDTV, COLOR_ROTATION_HDTV_TO_DCI_P3_D65 = 0, 1, 2   # ::ColorPrimaryRotation
COLOR_ROTATIONS = {"hdtv_to_uhdtv": COLOR_ROTATION_HDTV_TO_UHDTV, "dci_p3_d65_to_uhdtv": COLOR_ROTATION_DCI_P3_D65_TO_UHDTV,
                   "hdtv_to_dci_p3_d65": COLOR_ROTATION_HDTV_TO_DCI_P3_D65}
POST_MAX_SIZE = 16384
POST_STAGES = 9
# outputs of pt_post_render (PtPostTextures): name -> (numpy dtype, channels)
POST_FORMATS = {"Color": ("<u2", 4), "BackBuffer": ("<u4", 1), "Display8": ("u1", 4)}


def check_post_processing_settings(s):
    """The range checks of pt_post_set_constants, on the float32 values the library receives: ValueError where it answers
    PT_ERROR_INVALID_ARGUMENT."""
    s = np.asarray(s).reshape(())
    w, h = (int(v) for v in s["RenderSize"])
    f = {k: float(np.float32(s[k])) for k in ("BloomStrength", "Exposure", "PaperWhiteNits")}
    if not (1 <= w <= POST_MAX_SIZE and 1 <= h <= POST_MAX_SIZE):
        raise ValueError(f"RenderSize must be 1..{POST_MAX_SIZE} on both axes")
    if int(s["IsBloomEnabled"]) > 1 or int(s["IsHDREnabled"]) > 1:
        raise ValueError("IsBloomEnabled / IsHDREnabled must be 0 or 1")
    if not 0.0 <= f["BloomStrength"] <= 1.0:
        raise ValueError("BloomStrength must be in [0, 1]")
    if int(s["ToneMappingOperator"]) not in TONE_MAP_OPERATORS.values():
        raise ValueError("unknown ToneMappingOperator")
    if not -10.0 <= f["Exposure"] <= 10.0:
        raise ValueError("Exposure must be in [-10, 10]")
    if not 50.0 <= f["PaperWhiteNits"] <= 10000.0:
        raise ValueError("PaperWhiteNits must be in [50, 10000]")
    if int(s["ColorPrimaryRotation"]) not in COLOR_ROTATIONS.values():
        raise ValueError("unknown ColorPrimaryRotation")
    return s


def post_bloom_size_ok(width, height):
    """pt_post_render's bloom-on size rule: five mips of the (W/2, H/2) pyramid need max(W/2, H/2) >= 16, and W, H >= 2."""
    return width >= 2 and height >= 2 and max(width, height) >= 32


def post_processing_settings(width, height, bloom=True, strength=0.05, operator="aces_filmic", exposure=0.0, hdr=False,
                             paper_white_nits=200.0, rotation="hdtv_to_uhdtv"):
    """PtPostProcessSettings with the reference's defaults (Source/MyAppData.h:305-333): bloom on at strength 0.05, ACES filmic at
    exposure 0, paper white 200 nits, Rec.709 -> Rec.2020. HDR is off by default here (the library has no display to ask).
    operator / rotation: a name of TONE_MAP_OPERATORS / COLOR_ROTATIONS or the enum value. Refuses what pt_post_set_constants refuses."""
    s = np.zeros((), POST_PROCESS_SETTINGS)
    s["RenderSize"] = (width, height)
    s["IsBloomEnabled"] = 1 if bloom else 0
    s["BloomStrength"] = strength
    s["IsHDREnabled"] = 1 if hdr else 0
    s["ToneMappingOperator"] = TONE_MAP_OPERATORS[operator] if isinstance(operator, str) else operator
    s["Exposure"] = exposure
    s["PaperWhiteNits"] = paper_white_nits
    s["ColorPrimaryRotation"] = COLOR_ROTATIONS[rotation] if isinstance(rotation, str) else rotation
    return check_post_processing_settings(s)


NRD_COMPOSITION_CONSTANTS = np.dtype({  # PtNRDCompositionConstants: NRDComposition::Constants (Shaders/NRDComposition.hlsl:3-9), 8 root constants
    "names": ["RenderSize", "IsPack", "Denoiser", "ReBLURHitDistance"], "formats": [("<u4", 2), "<u4", "<u4", ("<f4", 4)],
    "offsets": [0, 8, 12, 16], "itemsize": 32})
# PtNRDCompositionTextures member order (NRDComposition::Textures): nine pointers
NRD_COMPOSITION_TEXTURES = ["LinearDepth", "DiffuseAlbedo", "SpecularAlbedo", "NormalRoughness", "NoisyDiffuse", "NoisySpecular",
                            "DenoisedDiffuse", "DenoisedSpecular", "Radiance"]
NRD_REBLUR_HIT_DISTANCE_DEFAULTS = (3.0, 0.1, 20.0, -25.0)   # nrd::ReblurSettings().hitDistanceParameters, from memory (unpinned)
NRD_MAX_SIZE = 16384


def check_nrd_composition_constants(k):
    """The checks pt_nrd_composition_process makes on its constants: ValueError where it answers PT_ERROR_INVALID_ARGUMENT."""
    k = np.asarray(k).reshape(())
    w, h = (int(v) for v in k["RenderSize"])
    if not (1 <= w <= NRD_MAX_SIZE and 1 <= h <= NRD_MAX_SIZE):
        raise ValueError(f"RenderSize must be 1..{NRD_MAX_SIZE} on both axes")
    if int(k["IsPack"]) > 1:
        raise ValueError("IsPack must be 0 or 1")
    if int(k["Denoiser"]) > DENOISER_NRD_RELAX:
        raise ValueError("unknown Denoiser value")
    if not np.all(np.isfinite(k["ReBLURHitDistance"])):
        raise ValueError("ReBLURHitDistance must be finite")
    return k


def nrd_composition_constants(width, height, denoiser, is_pack, hit_distance=None):
    """PtNRDCompositionConstants. width, height: the size of the arrays passed (a sharded context: its band). hit_distance: the four
    ReBLUR hit-distance parameters, None: NRD_REBLUR_HIT_DISTANCE_DEFAULTS. Refuses what pt_nrd_composition_process refuses."""
    for name, v in (("RenderSize", width), ("RenderSize", height), ("Denoiser", denoiser), ("IsPack", int(is_pack))):
        if not 0 <= int(v) <= 0xFFFFFFFF:
            raise ValueError(f"{name} is not a 32-bit unsigned value")
    k = np.zeros((), NRD_COMPOSITION_CONSTANTS)
    k["RenderSize"] = (width, height)
    k["IsPack"] = int(is_pack)
    k["Denoiser"] = denoiser
    k["ReBLURHitDistance"] = NRD_REBLUR_HIT_DISTANCE_DEFAULTS if hit_distance is None else hit_distance
    return check_nrd_composition_constants(k)


DENOISER_SETTINGS = np.dtype({  # PtDenoiserSettings, 48 B
    "names": ["RenderSize", "MaxAccumulatedFrames", "AtrousIterations", "DepthThreshold", "NormalCosine", "DiffuseLuminanceSigma",
              "SpecularLuminanceSigma", "RoughnessFraction", "_pad"],
    "formats": [("<u4", 2), "<u4", "<u4", "<f4", "<f4", "<f4", "<f4", "<f4", ("<u4", 3)],
    "offsets": [0, 8, 12, 16, 20, 24, 28, 32, 36], "itemsize": 48})
# PtDenoiserTextures member order: eight pointers
DENOISER_TEXTURES = ["Position", "LinearDepth", "NormalRoughness", "MotionVector", "NoisyDiffuse", "NoisySpecular",
                     "DenoisedDiffuse", "DenoisedSpecular"]
DENOISER_DEFAULTS = {"MaxAccumulatedFrames": 30, "AtrousIterations": 5, "DepthThreshold": 0.01, "NormalCosine": 0.8,
                     "DiffuseLuminanceSigma": 2.0, "SpecularLuminanceSigma": 1.0, "RoughnessFraction": 0.15}
DENOISER_MAX_SIZE = 16384


def check_denoiser_settings(s):
    """The range checks of pt_denoiser_set_constants, on the float32 values the library receives: ValueError where it answers
    PT_ERROR_INVALID_ARGUMENT."""
    s = np.asarray(s).reshape(())
    w, h = (int(v) for v in s["RenderSize"])
    f = {k: float(np.float32(s[k])) for k in ("DepthThreshold", "NormalCosine", "DiffuseLuminanceSigma", "SpecularLuminanceSigma", "RoughnessFraction")}
    if not (1 <= w <= DENOISER_MAX_SIZE and 1 <= h <= DENOISER_MAX_SIZE):
        raise ValueError(f"RenderSize must be 1..{DENOISER_MAX_SIZE} on both axes")
    if not 1 <= int(s["MaxAccumulatedFrames"]) <= 255:
        raise ValueError("MaxAccumulatedFrames must be 1..255")
    if int(s["AtrousIterations"]) > 8:
        raise ValueError("AtrousIterations must be 0..8")
    if not 0.0 < f["DepthThreshold"] <= 1.0:
        raise ValueError("DepthThreshold must be in (0, 1]")
    if not 0.0 <= f["NormalCosine"] < 1.0:
        raise ValueError("NormalCosine must be in [0, 1)")
    for k in ("DiffuseLuminanceSigma", "SpecularLuminanceSigma", "RoughnessFraction"):
        if not (f[k] > 0.0 and np.isfinite(f[k])):
            raise ValueError(f"{k} must be positive and finite")
    return s


def denoiser_settings(width, height, **overrides):
    """PtDenoiserSettings with the defaults of DENOISER_DEFAULTS; overrides by field name. Refuses what pt_denoiser_set_constants refuses."""
    s = np.zeros((), DENOISER_SETTINGS)
    for name, v in (("RenderSize", width), ("RenderSize", height)):
        if not 0 <= int(v) <= 0xFFFFFFFF:
            raise ValueError(f"{name} is not a 32-bit unsigned value")
    s["RenderSize"] = (width, height)
    values = dict(DENOISER_DEFAULTS)
    for k, v in overrides.items():
        if k not in values:
            raise ValueError(f"PtDenoiserSettings has no field {k}")
        values[k] = v
    for k, v in values.items():
        if s.dtype[k].kind == "u" and not 0 <= int(v) <= 0xFFFFFFFF:
            raise ValueError(f"{k} is not a 32-bit unsigned value")
        s[k] = v
    return check_denoiser_settings(s)


UPSCALER_SETTINGS = np.dtype({  # PtUpscalerSettings, 48 B
    "names": ["RenderSize", "OutputSize", "MaxAccumulatedFrames", "KernelRadius", "DepthThreshold", "_pad"],
    "formats": [("<u4", 2), ("<u4", 2), "<u4", "<f4", "<f4", ("<u4", 5)],
    "offsets": [0, 8, 16, 20, 24, 28], "itemsize": 48})
# PtUpscalerTextures member order: four pointers
UPSCALER_TEXTURES = ["Radiance", "LinearDepth", "MotionVector", "Color"]
UPSCALER_DEFAULTS = {"MaxAccumulatedFrames": 16, "KernelRadius": 1.0, "DepthThreshold": 0.01}
UPSCALER_MAX_SIZE = 16384
# PtSuperResolutionMode, SuperResolutionMode of Source/Upscaler.ixx in its order
SUPER_RESOLUTION_AUTO, SUPER_RESOLUTION_NATIVE, SUPER_RESOLUTION_QUALITY, SUPER_RESOLUTION_BALANCED = 0, 1, 2, 3
SUPER_RESOLUTION_PERFORMANCE, SUPER_RESOLUTION_ULTRA_PERFORMANCE = 4, 5
SUPER_RESOLUTION_RATIO10 = {SUPER_RESOLUTION_NATIVE: 10, SUPER_RESOLUTION_QUALITY: 15, SUPER_RESOLUTION_BALANCED: 17,
                            SUPER_RESOLUTION_PERFORMANCE: 20, SUPER_RESOLUTION_ULTRA_PERFORMANCE: 30}


def check_upscaler_settings(s):
    """The range checks of pt_upscaler_set_constants, on the float32 values the library receives: ValueError where it answers
    PT_ERROR_INVALID_ARGUMENT."""
    s = np.asarray(s).reshape(())
    render, output = [int(v) for v in s["RenderSize"]], [int(v) for v in s["OutputSize"]]
    for name, size in (("RenderSize", render), ("OutputSize", output)):
        if not all(1 <= v <= UPSCALER_MAX_SIZE for v in size):
            raise ValueError(f"{name} must be 1..{UPSCALER_MAX_SIZE} on both axes")
    if not all(r <= o <= 4 * r for r, o in zip(render, output)):
        raise ValueError("OutputSize must be RenderSize..4 RenderSize on both axes")
    if not 1 <= int(s["MaxAccumulatedFrames"]) <= 255:
        raise ValueError("MaxAccumulatedFrames must be 1..255")
    if not 0.75 <= float(np.float32(s["KernelRadius"])) <= 2.0:
        raise ValueError("KernelRadius must be in [0.75, 2]")
    if not 0.0 < float(np.float32(s["DepthThreshold"])) <= 1.0:
        raise ValueError("DepthThreshold must be in (0, 1]")
    return s


def upscaler_settings(render_size, output_size, **overrides):
    """PtUpscalerSettings with the defaults of UPSCALER_DEFAULTS; overrides by field name. Refuses what pt_upscaler_set_constants refuses."""
    s = np.zeros((), UPSCALER_SETTINGS)
    for name, size in (("RenderSize", render_size), ("OutputSize", output_size)):
        if len(size) != 2 or not all(0 <= int(v) <= 0xFFFFFFFF for v in size):
            raise ValueError(f"{name} is not a pair of 32-bit unsigned values")
        s[name] = tuple(int(v) for v in size)
    values = dict(UPSCALER_DEFAULTS)
    for k, v in overrides.items():
        if k not in values:
            raise ValueError(f"PtUpscalerSettings has no field {k}")
        values[k] = v
    for k, v in values.items():
        if s.dtype[k].kind == "u" and not 0 <= int(v) <= 0xFFFFFFFF:
            raise ValueError(f"{k} is not a 32-bit unsigned value")
        s[k] = v
    return check_upscaler_settings(s)


def upscaler_render_size(mode, output_size):
    """pt_upscaler_render_size restated: the render size of a PtSuperResolutionMode for an output size, in integers. No GPU."""
    mode, output = int(mode), [int(v) for v in output_size]
    if not SUPER_RESOLUTION_AUTO <= mode <= SUPER_RESOLUTION_ULTRA_PERFORMANCE:
        raise ValueError("mode must be a PtSuperResolutionMode value")
    if len(output) != 2 or not all(1 <= v <= UPSCALER_MAX_SIZE for v in output):
        raise ValueError(f"output must be 1..{UPSCALER_MAX_SIZE} on both axes")
    if mode == SUPER_RESOLUTION_AUTO:                  # by the pixel count of the output (App.cpp:1427-1440)
        pixels = output[0] * output[1]
        mode = (SUPER_RESOLUTION_NATIVE if pixels <= 1280 * 800 else SUPER_RESOLUTION_QUALITY if pixels <= 1920 * 1200
                else SUPER_RESOLUTION_BALANCED if pixels <= 2560 * 1600 else SUPER_RESOLUTION_PERFORMANCE if pixels <= 3840 * 2400
                else SUPER_RESOLUTION_ULTRA_PERFORMANCE)
    r10 = SUPER_RESOLUTION_RATIO10[mode]
    return tuple(max(1, (v * 10 + r10 // 2) // r10) for v in output)


def upscaler_jitter(frame_index, render_size, output_size):
    """pt_upscaler_jitter restated bit for bit: the Halton point (bases 2 and 3) of index frame_index % count + 1 minus 0.5, as two
    float32; count = ceil(8 (ow / rw) (oh / rh)) in float32. No GPU."""
    f32 = np.float32
    render, output = [int(v) for v in render_size], [int(v) for v in output_size]
    if len(render) != 2 or len(output) != 2 or not all(1 <= v <= UPSCALER_MAX_SIZE for v in render + output):
        raise ValueError(f"render and output must be 1..{UPSCALER_MAX_SIZE} on both axes")
    scaled = f32(f32(8) * f32(f32(output[0]) / f32(render[0])))
    count = int(np.ceil(f32(scaled * f32(f32(output[1]) / f32(render[1])))))
    index = int(frame_index) % count + 1
    out = []
    for base in (2, 3):
        inv = f32(1) / f32(base)
        weight, value, i = inv, f32(0), index
        while i > 0:
            value = f32(value + f32(f32(i % base) * weight))
            weight = f32(weight * inv)
            i //= base
        out.append(f32(value - f32(0.5)))
    return tuple(out)


RECONSTRUCTION_SETTINGS = np.dtype({  # PtReconstructionSettings, 64 B
    "names": ["RenderSize", "OutputSize", "MaxAccumulatedFrames", "MaxOutputFrames", "AtrousIterations", "DepthThreshold", "NormalCosine",
              "LuminanceSigma", "RoughnessFraction", "KernelRadius", "_pad"],
    "formats": [("<u4", 2), ("<u4", 2), "<u4", "<u4", "<u4", "<f4", "<f4", "<f4", "<f4", "<f4", ("<u4", 4)],
    "offsets": [0, 8, 16, 20, 24, 28, 32, 36, 40, 44, 48], "itemsize": 64})
# PtReconstructionTextures member order: eight pointers
RECONSTRUCTION_TEXTURES = ["Radiance", "DiffuseAlbedo", "SpecularAlbedo", "NormalRoughness", "Position", "LinearDepth", "MotionVector", "Color"]
RECONSTRUCTION_DEFAULTS = {"MaxAccumulatedFrames": 30, "MaxOutputFrames": 16, "AtrousIterations": 5, "DepthThreshold": 0.01,
                           "NormalCosine": 0.8, "LuminanceSigma": 2.0, "RoughnessFraction": 0.15, "KernelRadius": 1.0}
RECONSTRUCTION_MAX_SIZE = 16384
RECONSTRUCTION_FORM_DIRECT, RECONSTRUCTION_FORM_STAGED = 0x8000, 0x10000      # PT_RECONSTRUCTION_FORM_*: bits of pt_set_debug_flags


def check_reconstruction_settings(s):
    """The range checks of pt_reconstruction_set_constants, on the float32 values the library receives: ValueError where it answers
    PT_ERROR_INVALID_ARGUMENT."""
    s = np.asarray(s).reshape(())
    render, output = [int(v) for v in s["RenderSize"]], [int(v) for v in s["OutputSize"]]
    f = {k: float(np.float32(s[k])) for k in ("DepthThreshold", "NormalCosine", "LuminanceSigma", "RoughnessFraction", "KernelRadius")}
    for name, size in (("RenderSize", render), ("OutputSize", output)):
        if not all(1 <= v <= RECONSTRUCTION_MAX_SIZE for v in size):
            raise ValueError(f"{name} must be 1..{RECONSTRUCTION_MAX_SIZE} on both axes")
    if not all(r <= o <= 4 * r for r, o in zip(render, output)):
        raise ValueError("OutputSize must be RenderSize..4 RenderSize on both axes")
    for k in ("MaxAccumulatedFrames", "MaxOutputFrames"):
        if not 1 <= int(s[k]) <= 255:
            raise ValueError(f"{k} must be 1..255")
    if int(s["AtrousIterations"]) > 8:
        raise ValueError("AtrousIterations must be 0..8")
    if not 0.0 < f["DepthThreshold"] <= 1.0:
        raise ValueError("DepthThreshold must be in (0, 1]")
    if not 0.0 <= f["NormalCosine"] < 1.0:
        raise ValueError("NormalCosine must be in [0, 1)")
    for k in ("LuminanceSigma", "RoughnessFraction"):
        if not (f[k] > 0.0 and np.isfinite(f[k])):
            raise ValueError(f"{k} must be positive and finite")
    if not 0.75 <= f["KernelRadius"] <= 2.0:
        raise ValueError("KernelRadius must be in [0.75, 2]")
    return s


def reconstruction_settings(render_size, output_size, **overrides):
    """PtReconstructionSettings with the defaults of RECONSTRUCTION_DEFAULTS; overrides by field name. Refuses what
    pt_reconstruction_set_constants refuses."""
    s = np.zeros((), RECONSTRUCTION_SETTINGS)
    for name, size in (("RenderSize", render_size), ("OutputSize", output_size)):
        if len(size) != 2 or not all(0 <= int(v) <= 0xFFFFFFFF for v in size):
            raise ValueError(f"{name} is not a pair of 32-bit unsigned values")
        s[name] = tuple(int(v) for v in size)
    values = dict(RECONSTRUCTION_DEFAULTS)
    for k, v in overrides.items():
        if k not in values:
            raise ValueError(f"PtReconstructionSettings has no field {k}")
        values[k] = v
    for k, v in values.items():
        if s.dtype[k].kind == "u" and not 0 <= int(v) <= 0xFFFFFFFF:
            raise ValueError(f"{k} is not a 32-bit unsigned value")
        s[k] = v
    return check_reconstruction_settings(s)


FRAME_GENERATION_SETTINGS = np.dtype({  # PtFrameGenerationSettings, 48 B
    "names": ["RenderSize", "OutputSize", "Phase", "DepthThreshold", "_pad"],
    "formats": [("<u4", 2), ("<u4", 2), "<f4", "<f4", ("<u4", 6)],
    "offsets": [0, 8, 16, 20, 24], "itemsize": 48})
assert FRAME_GENERATION_SETTINGS.itemsize == 48
# PtFrameGenerationTextures member order: five pointers; Generated8 is optional
FRAME_GENERATION_TEXTURES = ["Color", "LinearDepth", "MotionVector", "Generated", "Generated8"]
FRAME_GENERATION_DEFAULTS = {"Phase": 0.5, "DepthThreshold": 0.01}
FRAME_GENERATION_MAX_SIZE = 16384
# PtFrameGenerationClass: the class byte of an output pixel
FRAME_GENERATION_BOTH, FRAME_GENERATION_CURRENT_ONLY, FRAME_GENERATION_PREVIOUS_ONLY, FRAME_GENERATION_FALLBACK = 0, 1, 2, 3
FRAME_GENERATION_EMPTY = 0xFFFFFFFFFFFFFFFF     # a cell of the midpoint field no surface landed in


def check_frame_generation_settings(s):
    """The range checks of pt_frame_generation_set_constants, on the float32 values the library receives: ValueError where it answers
    PT_ERROR_INVALID_ARGUMENT."""
    s = np.asarray(s).reshape(())
    render, output = [int(v) for v in s["RenderSize"]], [int(v) for v in s["OutputSize"]]
    for name, size in (("RenderSize", render), ("OutputSize", output)):
        if not all(1 <= v <= FRAME_GENERATION_MAX_SIZE for v in size):
            raise ValueError(f"{name} must be 1..{FRAME_GENERATION_MAX_SIZE} on both axes")
    if not all(r <= o <= 4 * r for r, o in zip(render, output)):
        raise ValueError("OutputSize must be RenderSize..4 RenderSize on both axes")
    if not 0.0 < float(np.float32(s["Phase"])) < 1.0:
        raise ValueError("Phase must be in (0, 1)")
    if not 0.0 < float(np.float32(s["DepthThreshold"])) <= 1.0:
        raise ValueError("DepthThreshold must be in (0, 1]")
    return s


def frame_generation_settings(render_size, output_size, **overrides):
    """PtFrameGenerationSettings with the defaults of FRAME_GENERATION_DEFAULTS; overrides by field name. Refuses what
    pt_frame_generation_set_constants refuses."""
    s = np.zeros((), FRAME_GENERATION_SETTINGS)
    for name, size in (("RenderSize", render_size), ("OutputSize", output_size)):
        if len(size) != 2 or not all(0 <= int(v) <= 0xFFFFFFFF for v in size):
            raise ValueError(f"{name} is not a pair of 32-bit unsigned values")
        s[name] = tuple(int(v) for v in size)
    values = dict(FRAME_GENERATION_DEFAULTS)
    for k, v in overrides.items():
        if k not in values:
            raise ValueError(f"PtFrameGenerationSettings has no field {k}")
        values[k] = v
    for k, v in values.items():
        s[k] = v
    return check_frame_generation_settings(s)


SHARPEN_SETTINGS = np.dtype({  # PtSharpenSettings, 32 B
    "names": ["Size", "Sharpness", "ContrastFloor", "_pad"],
    "formats": [("<u4", 2), "<f4", "<f4", ("<u4", 4)],
    "offsets": [0, 8, 12, 16], "itemsize": 32})
assert SHARPEN_SETTINGS.itemsize == 32
SHARPEN_TEXTURES = ["Color", "Sharpened"]       # PtSharpenTextures member order: two pointers
SHARPEN_DEFAULTS = {"Sharpness": 0.5, "ContrastFloor": 0.015625}
SHARPEN_MAX_SIZE = 16384
SHARPEN_MIN_CONTRAST_FLOOR = 2.0 ** -10


def check_sharpen_settings(s):
    """The range checks of pt_sharpen_set_constants, on the float32 values the library receives: ValueError where it answers
    PT_ERROR_INVALID_ARGUMENT (a value that is not finite is out of every range)."""
    s = np.asarray(s).reshape(())
    if not all(1 <= int(v) <= SHARPEN_MAX_SIZE for v in s["Size"]):
        raise ValueError(f"Size must be 1..{SHARPEN_MAX_SIZE} on both axes")
    if not 0.0 <= float(np.float32(s["Sharpness"])) <= 1.0:
        raise ValueError("Sharpness must be in [0, 1]")
    if not SHARPEN_MIN_CONTRAST_FLOOR <= float(np.float32(s["ContrastFloor"])) <= 0.5:
        raise ValueError("ContrastFloor must be in [2^-10, 0.5]")
    return s


def sharpen_settings(size, **overrides):
    """PtSharpenSettings with the defaults of SHARPEN_DEFAULTS; overrides by field name. Refuses what pt_sharpen_set_constants refuses."""
    s = np.zeros((), SHARPEN_SETTINGS)
    if len(size) != 2 or not all(0 <= int(v) <= 0xFFFFFFFF for v in size):
        raise ValueError("Size is not a pair of 32-bit unsigned values")
    s["Size"] = tuple(int(v) for v in size)
    values = dict(SHARPEN_DEFAULTS)
    for k, v in overrides.items():
        if k not in values:
            raise ValueError(f"PtSharpenSettings has no field {k}")
        values[k] = v
    for k, v in values.items():
        s[k] = v
    return check_sharpen_settings(s)


SHARC_SETTINGS = np.dtype({  # PtSHARCSettings: SHARC::Constants + Raytracing::SHARCSettings (Source/MyAppData.h:250-262)
    "names": ["AccumulationFrames", "MaxStaleFrames", "SceneScale", "IsAntiFireflyEnabled", "DownscaleFactor", "RoughnessThreshold",
              "IsHashGridVisualizationEnabled"],
    "formats": ["<u4", "<u4", "<f4", "<u4", "<u4", "<f4", "<u4"], "offsets": [0, 4, 8, 12, 16, 20, 24], "itemsize": 28})
SHARC_DEFAULT_CAPACITY = 1 << 22
SHARC_ENTRY = np.dtype({  # PtSHARCEntry: a live entry of the resolved buffer
    "names": ["Key", "Voxel"], "formats": ["<u8", ("<u4", 4)], "offsets": [0, 8], "itemsize": 32})
SHARC_QUERY_RESULT = np.dtype({"names": ["Valid", "Radiance"], "formats": ["<u4", ("<f4", 3)], "offsets": [0, 4], "itemsize": 16})
SHARC_PATH_VERTEX = np.dtype({  # PtSHARCPathVertex: one bounce of one update path
    "names": ["Position", "Flags", "Normal", "Random", "Radiance", "KeyLo", "Throughput", "KeyHi"],
    "formats": [("<f4", 3), "<u4", ("<f4", 3), "<f4", ("<f4", 3), "<u4", ("<f4", 3), "<u4"],
    "offsets": [0, 12, 16, 28, 32, 44, 48, 60], "itemsize": 64})
SHARC_PATH_SCATTER = np.dtype({  # PtSHARCPathScatter: the BSDF step of the same bounce; the first 96 bytes are a PtBsdfSampleQuery
    "names": ["Query", "Origin", "Sampled", "L", "Goes"], "formats": [("u1", 96), ("<f4", 3), "<u4", ("<f4", 3), "<u4"],
    "offsets": [0, 96, 108, 112, 124], "itemsize": 128})
SHARC_VERTEX_HIT, SHARC_VERTEX_MISS, SHARC_VERTEX_ENDED, SHARC_VERTEX_RESAMPLED = 1, 2, 4, 8
DEBUG_SHARC_LOG_PATHS, DEBUG_SHARC_SKIP_UPDATE = 0x100, 0x200


def check_sharc_settings(s):
    """The range checks of pt_sharc_set_constants, on the float32 values the library receives: ValueError where it answers
    PT_ERROR_INVALID_ARGUMENT."""
    s = np.asarray(s).reshape(())
    if not 1 <= int(s["DownscaleFactor"]) <= 4:
        raise ValueError("DownscaleFactor must be 1..4")
    if not 1 <= int(s["AccumulationFrames"]) <= 63:
        raise ValueError("AccumulationFrames must be 1..63")
    if not 1 <= int(s["MaxStaleFrames"]) <= 255:
        raise ValueError("MaxStaleFrames must be 1..255")
    if not 5.0 <= float(np.float32(s["SceneScale"])) <= 100.0:
        raise ValueError("SceneScale must be in [5, 100]")
    if not 0.0 <= float(np.float32(s["RoughnessThreshold"])) <= 1.0:
        raise ValueError("RoughnessThreshold must be in [0, 1]")
    if int(s["IsAntiFireflyEnabled"]) > 1:
        raise ValueError("IsAntiFireflyEnabled must be 0 or 1")
    if int(s["IsHashGridVisualizationEnabled"]) != 0:
        raise ValueError("hash-grid visualisation is not served")
    return s


def sharc_settings(downscale=4, scene_scale=50.0, roughness_threshold=0.4, accumulation_frames=10, max_stale_frames=64,
                   anti_firefly=True, visualization=False):
    """PtSHARCSettings with the reference's defaults (Source/MyAppData.h:250-262, Source/SHARC.ixx): DownscaleFactor 4, SceneScale 50,
    RoughnessThreshold 0.4, 10 accumulation frames, 64 stale frames, anti-firefly on (the reference passes true). Refuses what
    pt_sharc_set_constants refuses."""
    s = np.zeros((), SHARC_SETTINGS)
    s["AccumulationFrames"] = accumulation_frames
    s["MaxStaleFrames"] = max_stale_frames
    s["SceneScale"] = scene_scale
    s["IsAntiFireflyEnabled"] = 1 if anti_firefly else 0
    s["DownscaleFactor"] = downscale
    s["RoughnessThreshold"] = roughness_threshold
    s["IsHashGridVisualizationEnabled"] = 1 if visualization else 0
    return check_sharc_settings(s)


GBUFFER_CONSTANTS = np.dtype({
    "names": ["RenderSize", "Flags"], "formats": [("<u4", 2), "<u4"], "offsets": [0, 8], "itemsize": 12})


class GBufferFlags:  # Shaders/GBufferGeneration.hlsl:9-28
    Position = 0x1
    FlatNormal = 0x2
    GeometricNormal = 0x4
    LinearDepth = 0x8
    NormalizedDepth = 0x10
    MotionVector = 0x20
    DiffuseAlbedo = 0x40
    SpecularAlbedo = 0x80
    Albedo = 0xC0
    NormalRoughness = 0x100
    Radiance = 0x200
    Geometry = 0x1 | 0x2 | 0x4 | 0x8 | 0x10 | 0x20 | 0x100
    Material = 0x400 | 0xC0 | 0x100 | 0x200
    # what App.cpp:1224 passes when the denoiser is None
    DefaultNoDenoiser = 0xFFFFFFFF & ~0xC0


# G-buffer texture formats (Source/App.cpp:438-455): name -> (numpy dtype, channels)
GBUFFER_FORMATS = {
    "Position": ("<f4", 4),            # RGBA32F
    "FlatNormal": ("<i2", 2),          # RG16_SNORM
    "GeometricNormal": ("<i2", 2),     # RG16_SNORM
    "LinearDepth": ("<f4", 1),         # R32F
    "NormalizedDepth": ("<f4", 1),     # R32F
    "MotionVector": ("<u2", 4),        # RGBA16F (raw half bits)
    "BaseColorMetalness": ("u1", 4),   # RGBA8_UNORM
    "DiffuseAlbedo": ("<u2", 4),       # RGBA16F, written when a denoiser is selected
    "SpecularAlbedo": ("<u2", 4),      # RGBA16F, written when a denoiser is selected
    "NormalRoughness": ("<i2", 4),     # RGBA16_SNORM
    "IOR": ("<u2", 1),                 # R16F
    "Transmission": ("u1", 1),         # R8_UNORM
    "Radiance": ("<u2", 4),            # RGBA16F
}
GBUFFER_ORDER = list(GBUFFER_FORMATS.keys())
# denoiser-facing outputs of the path tracer (Source/App.cpp:475-482)
DENOISER_FORMATS = {"Diffuse": ("<u2", 4), "Specular": ("<u2", 4), "SpecularHitDistance": ("<u2", 1)}
DENOISER_NONE, DENOISER_DLSS_RR, DENOISER_NRD_REBLUR, DENOISER_NRD_RELAX = 0, 1, 2, 3     # Source/Denoiser.ixx:8


def default_material():
    """Material() defaults, Source/Material.ixx:13-19."""
    m = np.zeros((), MATERIAL)
    m["BaseColor"] = (0, 0, 0, 1)
    m["EmissiveStrength"] = 1
    m["Roughness"] = 0.5
    m["IOR"] = 1.5
    m["AlphaCutoff"] = 0.5
    return m
