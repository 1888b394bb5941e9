// ptamd.hpp -- C++ host-side mirror of the reference's operators over the C ABI (include/ptamd.h).
//
// Same names, members and call order as the reference structs this path replaces, so that
// App::RenderScene (Source/App.cpp:1157-1329) keeps its shape when it is pointed at the MI355X path:
//     struct GBufferGeneration   Source/GBufferGeneration.ixx:27-122
//     struct Raytracing          Source/Raytracing.ixx:29-250      (DEFAULT permutation, and the SHARC overload with struct SHARC)
//     BuildTopLevelAccelerationStructure / CreateGeometryDesc       Source/RaytracingHelpers.ixx:28-105
//     struct SkeletalMeshSkinning Source/SkeletalMeshSkinning.ixx:20-66
//     struct Animation / AnimationCollection   Source/Animation.ixx:78-197 (the clock and the selection; the transforms are computed on the device)
//     struct PostProcessing      App::PostProcessGraphics with Denoiser::None (Source/App.cpp:1506-1571): Bloom, Merge, ToneMap, CopyTexture
//     struct NRDComposition      Source/NRDComposition.ixx (the pack and compose passes of App::ProcessNRD, Source/App.cpp:1595-1688)
//     struct Denoiser            the library's own filter for the ReLAX slot between them (where the reference calls NRD::Denoise)
//     struct Upscaler            the library's own temporal upscaler for the super-resolution step (where the reference calls DLSS or XeSS)
//     struct Reconstruction      the library's own denoising upscaler for the ray-reconstruction step (where the reference calls DLSS-RR)
//     struct FrameGeneration     the library's own frame interpolator for the frame-generation step (where the reference calls DLSS-G)
//     struct Sharpening          the library's own adaptive sharpener for the image-scaling step (where the reference calls NIS)
// Error behaviour: a failing status becomes the exception type the reference throws at the same place
// (std::invalid_argument for argument checks, std::system_error otherwise: Source/ErrorHelpers.ixx:16-32).
// Header-only, plain C++20 (std::span), no HIP headers needed by the including translation unit.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <memory>
#include <span>
#include <stdexcept>
#include <string>
#include <system_error>
#include <vector>

#include "../../include/ptamd.h"

namespace ptamd {

inline void ThrowIfFailed(PtContext* ctx, int status)
{
    if (status == PT_OK) return;
    std::string msg = pt_last_error(ctx);
    if (status == PT_ERROR_INVALID_ARGUMENT) throw std::invalid_argument(msg);
    throw std::system_error(status, std::generic_category(), msg);
}

// Stand-in for the reference's DeviceContext + CommandList pair: one HIP device + one stream.
struct CommandList {
    PtContext* Context = nullptr;

    explicit CommandList(int deviceOrdinal = 0, void* hipStream = nullptr)
    {
        int s = pt_create(deviceOrdinal, &Context);
        if (s != PT_OK) throw std::system_error(s, std::generic_category(), pt_last_error(nullptr));
        if (hipStream) ThrowIfFailed(Context, pt_set_stream(Context, hipStream));
    }
    CommandList(const CommandList&) = delete;
    CommandList& operator=(const CommandList&) = delete;
    ~CommandList() { pt_destroy(Context); }

    void End() { ThrowIfFailed(Context, pt_sync(Context)); }            // CommandList::End + Wait, Source/CommandList.ixx:86-119

    // Frames in flight: this command list renders the scene `owner` built (acceleration structures, descriptor table, object and
    // instance data), read-only, on its own stream with its own path queues. The reference has ONE Scene whatever the number of
    // frames in flight (Source/App.cpp:372-374). `owner` must outlive the sharing.
    void ShareScene(const CommandList& owner) { ThrowIfFailed(Context, pt_share_scene(Context, owner.Context)); }
};

// Multi-GPU (no reference counterpart: the reference presents from one device). One process per GPU; every rank renders its 16-row
// bands (pt_set_sharding) and the root assembles the frame with one grouped RCCL exchange over xGMI (pt_gather_bands).
struct BandSharding {
    static constexpr uint32_t BandHeight = 16;
    uint32_t Rank = 0, World = 1;

    // every rank calls this with the same 128-byte id (UniqueId() of one rank, distributed by the caller); returns when all have joined
    void Join(CommandList& commandList, uint32_t rank, uint32_t world, const void* uniqueId)
    {
        Rank = rank; World = world;
        const PtSharding s{ rank, world, BandHeight, 0 };
        ThrowIfFailed(commandList.Context, pt_set_sharding(commandList.Context, &s));
        if (world > 1 || uniqueId) ThrowIfFailed(commandList.Context, pt_comm_init(commandList.Context, uniqueId, rank, world));
    }
    static std::vector<uint8_t> UniqueId()
    {
        std::vector<uint8_t> id(PT_COMM_ID_BYTES);
        int s = pt_comm_get_unique_id(id.data());
        if (s != PT_OK) throw std::system_error(s, std::generic_category(), pt_last_error(nullptr));
        return id;
    }
    uint32_t LocalRows(uint32_t height) const
    {
        const PtSharding s{ Rank, World, BandHeight, 0 };
        uint32_t rows = 0;
        if (pt_local_rows(&s, height, &rows) != PT_OK) throw std::invalid_argument("invalid sharding");
        return rows;
    }
    // localTexture: this rank's rows of a texture; fullFrame (root only): H x W pixels. Enqueued on the command list's stream.
    void GatherBands(CommandList& commandList, const void* localTexture, void* fullFrame, uint32_t width, uint32_t height, uint32_t pixelBytes, uint32_t root = 0)
    {
        ThrowIfFailed(commandList.Context, pt_gather_bands(commandList.Context, localTexture, fullFrame, width, height, pixelBytes, root));
    }
};

// GPUBuffer* / Texture* slots of the reference become plain device pointers here.
struct GPUBuffer { const void* DevicePointer = nullptr; uint64_t Capacity = 0; uint32_t Stride = 0; };

namespace RaytracingHelpers {

// CreateGeometryDesc, Source/RaytracingHelpers.ixx:76-105 (same argument checks, same exception texts)
inline PtGeometryDesc CreateGeometryDesc(const GPUBuffer& vertices, const GPUBuffer& indices, uint32_t flags = 0)
{
    if (indices.Stride != sizeof(uint16_t) && indices.Stride != sizeof(uint32_t))
        throw std::invalid_argument("Triangle index format must be either uint16 or uint32");
    if (indices.Capacity % 3 != 0) throw std::invalid_argument("Triangle index count must be divisible by 3");
    PtGeometryDesc d{};
    d.VertexBuffer = vertices.DevicePointer; d.VertexCount = (uint32_t)vertices.Capacity; d.VertexStride = vertices.Stride;
    d.IndexBuffer = indices.DevicePointer; d.IndexCount = (uint32_t)indices.Capacity; d.IndexStride = indices.Stride;
    d.Flags = flags;
    return d;
}

struct TopLevelAccelerationStructure { bool Valid = false; };

// BuildTopLevelAccelerationStructure, Source/RaytracingHelpers.ixx:28-74
inline void BuildTopLevelAccelerationStructure(CommandList& commandList, uint32_t flags, std::span<const PtInstanceDesc> descs,
                                               bool /*resize*/, TopLevelAccelerationStructure& accelerationStructure)
{
    ThrowIfFailed(commandList.Context, pt_build_top_level(commandList.Context, descs.data(), (uint32_t)descs.size(), flags));
    accelerationStructure.Valid = true;
}

// CommandList::BuildAccelerationStructures for one bottom-level input, Source/CommandList.ixx:217-233
inline uint64_t BuildBottomLevelAccelerationStructure(CommandList& commandList, std::span<const PtGeometryDesc> geometryDescs, uint32_t flags)
{
    uint64_t id = 0;
    ThrowIfFailed(commandList.Context, pt_build_bottom_level(commandList.Context, geometryDescs.data(), (uint32_t)geometryDescs.size(), flags, &id));
    return id;
}

// CommandList::UpdateAccelerationStructures for one bottom-level input (PERFORM_UPDATE after skinning), Source/CommandList.ixx:235-241
inline void UpdateBottomLevelAccelerationStructure(CommandList& commandList, uint64_t id, std::span<const PtGeometryDesc> geometryDescs, uint32_t flags)
{
    ThrowIfFailed(commandList.Context, pt_update_bottom_level(commandList.Context, id, geometryDescs.data(), (uint32_t)geometryDescs.size(), flags));
}

// RTXMU RemoveAccelerationStructures in ~Scene / CollectGarbage, Source/Scene.ixx:108-123
inline void ReleaseBottomLevelAccelerationStructure(CommandList& commandList, uint64_t id)
{
    ThrowIfFailed(commandList.Context, pt_release_bottom_level(commandList.Context, id));
}

} // namespace RaytracingHelpers

// The shader-visible descriptor heap (DeviceContext::ResourceDescriptorHeap): slots that ObjectData / SceneData index.
struct DescriptorHeap {
    explicit DescriptorHeap(CommandList& commandList, uint32_t capacity) : m_context(commandList.Context)
    {
        ThrowIfFailed(m_context, pt_heap_resize(m_context, capacity));
    }
    // GPUBuffer::CreateSRV(Raw|Structured|Typed), Source/GPUBuffer.ixx: vertex / index / motion-vector buffers (App.cpp:1046-1050)
    void SetBuffer(uint32_t descriptor, const GPUBuffer& buffer)
    {
        ThrowIfFailed(m_context, pt_heap_set_buffer(m_context, descriptor, buffer.DevicePointer, buffer.Capacity * buffer.Stride, buffer.Stride));
    }
    // Texture::CreateSRV for a material map or the environment map (App.cpp:1021-1024,1052-1063); mip 0 texels, cube = 6 faces.
    // format is a PtFormat: RGBA8 / RGBA8_SRGB / RGBA32F texel arrays, or PT_FORMAT_BC1 / BC3 / BC4 / BC5_*: the tightly packed 4x4 blocks of a
    // DDS file's mip 0 as they are (2D only, 8- / 16-byte aligned), sampled in place
    void SetTexture(uint32_t descriptor, const void* texels, uint32_t width, uint32_t height, PtFormat format, bool isCubeMap = false)
    {
        ThrowIfFailed(m_context, pt_heap_set_texture(m_context, descriptor, texels, width, height, (uint32_t)format, isCubeMap ? 1u : 0u));
    }
private:
    PtContext* m_context;
};

// struct SkeletalMeshSkinning, Source/SkeletalMeshSkinning.ixx:20-66 (Prepare has nothing to bind here)
struct SkeletalMeshSkinning {
    struct { const GPUBuffer* SkeletalVertices; const GPUBuffer* SkeletalTransforms; const GPUBuffer* Vertices; const GPUBuffer* MotionVectors; } GPUBuffers{};

    explicit SkeletalMeshSkinning(CommandList&) {}
    void Prepare(CommandList&) {}
    void Process(CommandList& commandList)                  // :43-65, vertexCount = Vertices->GetCapacity()
    {
        if (!GPUBuffers.SkeletalVertices || !GPUBuffers.SkeletalTransforms || !GPUBuffers.Vertices || !GPUBuffers.MotionVectors)
            throw std::invalid_argument("SkeletalMeshSkinning::GPUBuffers not set");
        ThrowIfFailed(commandList.Context, pt_skin_mesh(commandList.Context, GPUBuffers.SkeletalVertices->DevicePointer,
                                                        (const float*)GPUBuffers.SkeletalTransforms->DevicePointer,
                                                        const_cast<void*>(GPUBuffers.Vertices->DevicePointer),
                                                        const_cast<void*>(GPUBuffers.MotionVectors->DevicePointer),
                                                        (uint32_t)GPUBuffers.Vertices->Capacity));
    }
};

// ---- animation (Source/Animation.ixx). The reference's Animation computes its transforms on the CPU in Tick; here Tick and SetTime keep the clock
// only, and AnimationCollection::Evaluate hands the selected clips and their times to the device (pt_anim_evaluate), which leaves the global
// transforms, the skeletal transforms of every skin and the posed InstanceData where skinning and the top-level build read them.
struct AnimationRig {                   // one animation file on the device: node forest, clips and keys, names resolved to indices by the loader
    struct Desc {                       // the arrays of pt_anim_create_rig
        std::span<const int32_t> Parents; std::span<const float> RestTRS; std::span<const double> Durations; std::span<const uint32_t> Channels;
        std::span<const float> KeyTimes, KeyValues;
    };
    uint64_t ID = 0; std::vector<double> Durations;
    AnimationRig(CommandList& commandList, const Desc& d) : Durations(d.Durations.begin(), d.Durations.end()), m_context(commandList.Context)
    {
        ThrowIfFailed(m_context, pt_anim_create_rig(m_context, (uint32_t)d.Parents.size(), d.Parents.data(), d.RestTRS.data(), (uint32_t)d.Durations.size(), d.Durations.data(),
                                                    d.Channels.data(), d.KeyTimes.data(), d.KeyValues.data(), (uint32_t)d.KeyTimes.size(), &ID));
    }
    AnimationRig(const AnimationRig&) = delete;
    AnimationRig& operator=(const AnimationRig&) = delete;
    ~AnimationRig() { pt_anim_release_rig(m_context, ID); }
private:
    PtContext* m_context;
};

struct Animation {                      // one clip: Source/Animation.ixx:78-175
    std::string Name;
    explicit Animation(double duration) : m_duration(duration) {}
    auto GetDuration() const { return m_duration; }
    auto GetTime() const { return m_time; }
    void SetTime(double seconds = 0) { m_time = std::clamp(seconds, 0.0, m_duration); }                       // :107
    void Tick(double elapsedSeconds) { m_time = m_duration > 0 ? std::fmod(m_time + elapsedSeconds, m_duration) : 0.0; }   // :109-113; Duration 0 stays at 0 (the reference: NaN)
private:
    double m_duration, m_time{};
};

struct AnimationCollection : std::vector<Animation> {     // Source/Animation.ixx:177-197, bound to ONE render object (Scene.ixx:165-168)
    struct Bindings {                   // the arrays of pt_anim_create_object
        std::span<const float> Transform;                 // RenderObject.Transform(), 16 floats
        std::span<const uint32_t> Nodes, Instances; std::span<const float> GlobalTransforms;
        std::span<const uint32_t> SkinMeshNodes, SkinJointCounts, JointNodes; std::span<const float> InverseBindMatrices;
    };
    std::string Name;
    uint64_t Object = 0;

    AnimationCollection(CommandList& commandList, std::shared_ptr<AnimationRig> rig, const Bindings& b) : m_context(commandList.Context), m_rig(std::move(rig)), m_isSkinned(!b.SkinMeshNodes.empty())
    {
        for (double d : m_rig->Durations) emplace_back(d);
        ThrowIfFailed(m_context, pt_anim_create_object(m_context, m_rig->ID, b.Transform.data(), (uint32_t)b.Nodes.size(), b.Nodes.data(), b.Instances.data(), b.GlobalTransforms.data(),
                                                       (uint32_t)b.SkinMeshNodes.size(), b.SkinMeshNodes.data(), b.SkinJointCounts.data(), b.JointNodes.data(), b.InverseBindMatrices.data(), &Object));
    }
    AnimationCollection(const AnimationCollection&) = delete;
    AnimationCollection& operator=(const AnimationCollection&) = delete;
    ~AnimationCollection() { pt_anim_release_object(m_context, Object); }

    auto GetSelectedIndex() const { return std::min(m_selectedIndex, size() - 1); }
    void SetSelectedIndex(size_t index) { m_selectedIndex = std::min(index, size() - 1); }
    auto IsSkinned() const { return m_isSkinned; }
    // Animation::GetSkeletalTransforms for one skinned mesh node: the device array SkeletalMeshSkinning::GPUBuffers.SkeletalTransforms takes
    GPUBuffer GetSkeletalTransforms(uint32_t skin) const
    {
        const float* p = nullptr; uint32_t joints = 0;
        ThrowIfFailed(m_context, pt_anim_skeletal_transforms(m_context, Object, skin, &p, &joints));
        return GPUBuffer{ p, joints, 48 };
    }
    // Animation::ComputeTransforms + Scene::Refresh for every collection of a scene in ONE launch, at each one's selected clip and time
    static void Evaluate(CommandList& commandList, std::span<AnimationCollection* const> collections, PtInstanceData* deviceInstances)
    {
        std::vector<PtAnimState> states;
        for (const AnimationCollection* c : collections) states.push_back(PtAnimState{ c->Object, (uint32_t)c->GetSelectedIndex(), 0, (*c)[c->GetSelectedIndex()].GetTime() });
        ThrowIfFailed(commandList.Context, pt_anim_evaluate(commandList.Context, states.data(), (uint32_t)states.size(), deviceInstances));
    }
private:
    PtContext* m_context;
    std::shared_ptr<AnimationRig> m_rig;
    size_t m_selectedIndex{};
    bool m_isSkinned{};
};

namespace RaytracingHelpers {
// BuildTopLevelAccelerationStructure over posed instances: where fromDevice[i] is set, instance i's transform is InstanceData[i].ObjectToWorld as
// AnimationCollection::Evaluate left it on the device
inline void BuildTopLevelAccelerationStructure(CommandList& commandList, uint32_t flags, std::span<const PtInstanceDesc> descs, const PtInstanceData* deviceInstances,
                                               std::span<const uint8_t> fromDevice, TopLevelAccelerationStructure& accelerationStructure)
{
    if (fromDevice.size() != descs.size()) throw std::invalid_argument("fromDevice must name every instance");
    ThrowIfFailed(commandList.Context, pt_build_top_level_posed(commandList.Context, descs.data(), (uint32_t)descs.size(), flags, deviceInstances, fromDevice.data()));
    accelerationStructure.Valid = true;
}
}

// The RTXDI operator of the reference (Source/RTXDI.ixx: SetConstants + Render) as this library restates it: direct lighting from the
// scene's emissive triangles, written to Textures.Diffuse / Specular for the path tracer (GraphicsSettings.IsDIEnabled), or added to
// Textures.Radiance when it is the last render pass. Also the two calls the reference's direct-lighting bridge makes on the same scene
// data (Shaders/RTXDIAppBridge.hlsli:418-439, Shaders/BxDF.hlsli:247-285), batched over device arrays.
struct DirectLighting {
    struct Settings {
        uint32_t RenderSize[2]{};
        uint32_t FrameIndex{}, LocalLightSamples = 8;        // 1..32
        uint32_t Denoiser{};
        bool IsLastRenderPass{};
        uint32_t ExtFlags{};
    };

    // MyAppData ReSTIRDI.TemporalResampling / SpatialResampling (Source/MyAppData.h:226-247); the thresholds, history length, radius and
    // disocclusion boost are the RTXDI SDK's documented defaults. Both passes off by default: the plain pass. Pairwise and Raytraced
    // (the reference's values 2 and 3) reach the library as BASIC plus pt_di_set_pairwise's / pt_di_set_visibility's flag of the pass.
    enum class ReSTIRDIBiasCorrectionMode : uint32_t { Off = PT_DI_BIAS_CORRECTION_OFF, Basic = PT_DI_BIAS_CORRECTION_BASIC, Pairwise = 2, Raytraced = 3 };
    struct ReSTIRDI {
        struct TemporalResampling {
            bool IsEnabled{};
            ReSTIRDIBiasCorrectionMode BiasCorrectionMode = ReSTIRDIBiasCorrectionMode::Basic;
            struct BoilingFilter { bool IsEnabled = true; float Strength = 0.2f; } BoilingFilter;
            uint32_t MaxHistoryLength = 20;
            float DepthThreshold = 0.1f, NormalThreshold = 0.5f;
        } TemporalResampling;
        struct SpatialResampling {
            bool IsEnabled{};
            ReSTIRDIBiasCorrectionMode BiasCorrectionMode = ReSTIRDIBiasCorrectionMode::Basic;
            uint32_t Samples = 1, DisocclusionBoostSamples = 8;
            float SamplingRadius = 32.0f, DepthThreshold = 0.1f, NormalThreshold = 0.5f;
        } SpatialResampling;
    };

    // MyAppData ReSTIRDI.InitialSampling.LocalLight.Mode and ReSTIRDI.ReGIR.{Cell.Size, BuildSamples} (Source/MyAppData.h:200-215).
    // PowerCDF, this library's default, is not a reference mode; the reference's default is ReGIR_RIS.
    enum class ReSTIRDILocalLightSamplingMode : uint32_t {
        PowerCDF = PT_DI_LOCAL_LIGHT_POWER_CDF, Uniform = PT_DI_LOCAL_LIGHT_UNIFORM, Power_RIS = PT_DI_LOCAL_LIGHT_POWER_RIS, ReGIR_RIS = PT_DI_LOCAL_LIGHT_REGIR_RIS
    };
    // ReGIRLayout: the cells' layout (pt_di_set_regir_layout). The reference compiles the Onion (Shaders/RTXDIAppBridge.hlsli:6); the Grid is
    // this library's default.
    enum class ReGIRLayout : uint32_t { Grid = PT_DI_REGIR_LAYOUT_GRID, Onion = PT_DI_REGIR_LAYOUT_ONION };
    struct LightSampling {
        struct InitialSampling { struct LocalLight { ReSTIRDILocalLightSamplingMode Mode = ReSTIRDILocalLightSamplingMode::ReGIR_RIS; } LocalLight; } InitialSampling;
        struct ReGIR {
            struct Cell { float Size = 1.0f; } Cell;       // [0.1, 10]
            uint32_t BuildSamples = 8;                      // 1..32
            ReGIRLayout Layout = ReGIRLayout::Grid;
        } ReGIR;
    };

    struct { const PtSceneData* SceneData; const PtCamera* Camera; const PtObjectData* ObjectData; uint32_t ObjectCount; } GPUBuffers{};
    PtTextures Textures{};                                  // the G-buffer it reads, Diffuse / Specular (or Radiance) it writes
    PtDIPreviousTextures PreviousTextures{};                // RTXDI::Textures Previous*: last frame's G-buffer (temporal resampling)

    explicit DirectLighting(CommandList& commandList) : m_context(commandList.Context) {}

    void SetResampling(const ReSTIRDI& r)
    {
        PtDIResamplingSettings s{};
        s.TemporalResampling = r.TemporalResampling.IsEnabled ? 1u : 0u;
        s.TemporalBiasCorrection = LibraryBiasCorrection(r.TemporalResampling.BiasCorrectionMode);
        s.MaxHistoryLength = r.TemporalResampling.MaxHistoryLength;
        s.BoilingFilter = r.TemporalResampling.BoilingFilter.IsEnabled ? 1u : 0u;
        s.BoilingFilterStrength = r.TemporalResampling.BoilingFilter.Strength;
        s.TemporalDepthThreshold = r.TemporalResampling.DepthThreshold; s.TemporalNormalThreshold = r.TemporalResampling.NormalThreshold;
        s.SpatialSamples = r.SpatialResampling.IsEnabled ? r.SpatialResampling.Samples : 0u;
        s.SpatialBiasCorrection = LibraryBiasCorrection(r.SpatialResampling.BiasCorrectionMode);
        s.DisocclusionBoostSamples = r.SpatialResampling.DisocclusionBoostSamples;
        s.SpatialSamplingRadius = r.SpatialResampling.SamplingRadius;
        s.SpatialDepthThreshold = r.SpatialResampling.DepthThreshold; s.SpatialNormalThreshold = r.SpatialResampling.NormalThreshold;
        ThrowIfFailed(m_context, pt_di_set_resampling(m_context, &s));
        PtDIPairwiseSettings p{};
        p.TemporalPairwise = r.TemporalResampling.BiasCorrectionMode == ReSTIRDIBiasCorrectionMode::Pairwise ? 1u : 0u;
        p.SpatialPairwise = r.SpatialResampling.BiasCorrectionMode == ReSTIRDIBiasCorrectionMode::Pairwise ? 1u : 0u;
        ThrowIfFailed(m_context, pt_di_set_pairwise(m_context, &p));
        m_temporalRaytraced = r.TemporalResampling.BiasCorrectionMode == ReSTIRDIBiasCorrectionMode::Raytraced;
        m_spatialRaytraced = r.SpatialResampling.BiasCorrectionMode == ReSTIRDIBiasCorrectionMode::Raytraced;
        ApplyVisibility();
    }

    void ResetHistory() { ThrowIfFailed(m_context, pt_di_reset_history(m_context)); }     // App::ResetHistory

    // Visibility in the reservoirs (pt_di_set_visibility): the RTXDI SDK's defaults, unpinned; it acts only with reuse on. The Raytraced
    // flags turn the Basic normalisation of a pass into ReSTIRDI_BiasCorrectionMode::Raytraced.
    struct Visibility {
        bool EnableInitialVisibility = true, ReuseFinalVisibility = true, DiscardInvisibleSamples = false;
        uint32_t FinalVisibilityMaxAge = 4;
        float FinalVisibilityMaxDistance = 16.0f;
        bool TemporalRaytraced = false, SpatialRaytraced = false;
    };
    void SetVisibility(const Visibility& v) { m_visibility = v; ApplyVisibility(); }

    void SetLightSampling(const LightSampling& l)
    {
        PtDILightSamplingSettings s{};
        s.Mode = (uint32_t)l.InitialSampling.LocalLight.Mode;
        s.ReGIRCellSize = l.ReGIR.Cell.Size; s.ReGIRBuildSamples = l.ReGIR.BuildSamples;
        ThrowIfFailed(m_context, pt_di_set_light_sampling(m_context, &s));
        PtDIReGIRLayoutSettings layout{};
        layout.Layout = (uint32_t)l.ReGIR.Layout;
        ThrowIfFailed(m_context, pt_di_set_regir_layout(m_context, &layout));
    }

    // MyAppData ReSTIRDI.InitialSampling.BRDFSamples (Source/MyAppData.h:220-221; reference default 1) and the BRDF ray cutoff
    // (pt_di_set_brdf_sampling). Samples 0, this library's default: no BRDF candidates.
    struct BrdfSampling { uint32_t Samples = 0; float Cutoff = 0.0f; };
    void SetBrdfSampling(const BrdfSampling& b)
    {
        ThrowIfFailed(m_context, pt_di_set_brdf_sampling(m_context, b.Samples, b.Cutoff));
    }

    // The LocalLightPDF texture of App::PrepareReSTIRDI (pt_di_set_pdf_mipmap): with it on every Render builds the texture and its mip
    // chain, and the Power_RIS / ReGIR modes descend the chain for their light tiles. Off, this library's default: the power prefix sum.
    void SetPdfMipmap(bool enabled) { ThrowIfFailed(m_context, pt_di_set_pdf_mipmap(m_context, enabled ? 1u : 0u)); }

    void SetConstants(const Settings& settings)
    {
        PtDISettings s{};
        s.RenderSize[0] = settings.RenderSize[0]; s.RenderSize[1] = settings.RenderSize[1];
        s.FrameIndex = settings.FrameIndex; s.LocalLightSamples = settings.LocalLightSamples; s.Denoiser = settings.Denoiser;
        s.IsLastRenderPass = settings.IsLastRenderPass ? 1u : 0u; s.ExtFlags = settings.ExtFlags;
        ThrowIfFailed(m_context, pt_di_set_constants(m_context, &s));
    }

    void Render(CommandList& commandList, const RaytracingHelpers::TopLevelAccelerationStructure& topLevelAccelerationStructure)
    {
        if (!topLevelAccelerationStructure.Valid) throw std::invalid_argument("top-level acceleration structure has not been built");
        PtContext* c = commandList.Context;
        ThrowIfFailed(c, pt_set_scene_data(c, GPUBuffers.SceneData));
        ThrowIfFailed(c, pt_set_camera(c, GPUBuffers.Camera));
        ThrowIfFailed(c, pt_set_object_data(c, GPUBuffers.ObjectData, GPUBuffers.ObjectCount));
        ThrowIfFailed(c, pt_di_render_with_history(c, &Textures, PreviousTextures.PreviousLinearDepth ? &PreviousTextures : nullptr));
    }

    static void TraceVisibility(CommandList& commandList, const PtRayDesc* deviceRays, uint32_t count, float* deviceVisibility)
    {
        ThrowIfFailed(commandList.Context, pt_trace_visibility(commandList.Context, deviceRays, count, deviceVisibility));
    }
    static void EvaluateBSDF(CommandList& commandList, const PtBsdfQuery* deviceQueries, uint32_t count, PtBsdfResult* deviceResults)
    {
        ThrowIfFailed(commandList.Context, pt_bsdf_evaluate(commandList.Context, deviceQueries, count, deviceResults));
    }

private:
    PtContext* m_context;
    static uint32_t LibraryBiasCorrection(ReSTIRDIBiasCorrectionMode m) { return m == ReSTIRDIBiasCorrectionMode::Off ? PT_DI_BIAS_CORRECTION_OFF : PT_DI_BIAS_CORRECTION_BASIC; }
    static Visibility NoVisibility() { Visibility v; v.EnableInitialVisibility = v.ReuseFinalVisibility = false; return v; }
    // the Visibility last set (none: every flag off) with the Raytraced modes of the last SetResampling on top
    void ApplyVisibility()
    {
        const Visibility& v = m_visibility;
        PtDIVisibilitySettings s{};
        s.InitialVisibility = v.EnableInitialVisibility ? 1u : 0u; s.FinalVisibilityReuse = v.ReuseFinalVisibility ? 1u : 0u;
        s.FinalVisibilityMaxAge = v.FinalVisibilityMaxAge; s.FinalVisibilityMaxDistance = v.FinalVisibilityMaxDistance;
        s.DiscardInvisibleSamples = v.DiscardInvisibleSamples ? 1u : 0u;
        s.TemporalRaytraced = v.TemporalRaytraced || m_temporalRaytraced ? 1u : 0u; s.SpatialRaytraced = v.SpatialRaytraced || m_spatialRaytraced ? 1u : 0u;
        ThrowIfFailed(m_context, pt_di_set_visibility(m_context, &s));
    }
    Visibility m_visibility = NoVisibility();
    bool m_temporalRaytraced = false, m_spatialRaytraced = false;
};

struct GBufferGeneration {
    struct Flags {                                          // Source/GBufferGeneration.ixx:28-44
        enum {
            Position = 0x1, FlatNormal = 0x2, GeometricNormal = 0x4, LinearDepth = 0x8, NormalizedDepth = 0x10,
            MotionVector = 0x20, DiffuseAlbedo = 0x40, SpecularAlbedo = 0x80, Albedo = DiffuseAlbedo | SpecularAlbedo,
            NormalRoughness = 0x100, Radiance = 0x200,
            Geometry = Position | FlatNormal | GeometricNormal | LinearDepth | NormalizedDepth | MotionVector | NormalRoughness,
            Material = 0x400 | Albedo | NormalRoughness | Radiance
        };
    };
    struct Constants { uint32_t RenderSize[2]{}; uint32_t Flags{}; };

    // SceneData / Camera: host structs (the reference copies them into constant buffers each frame,
    // Source/App.cpp:540-561,1016-1026); InstanceData / ObjectData: device arrays.
    struct { const PtSceneData* SceneData; const PtCamera* Camera; const PtInstanceData* InstanceData; const PtObjectData* ObjectData;
             uint32_t InstanceCount, ObjectCount; } GPUBuffers{};
    PtTextures Textures{};                                  // same member order as the reference's Textures struct

    explicit GBufferGeneration(CommandList& commandList) : m_context(commandList.Context) {}

    void Render(CommandList& commandList, const RaytracingHelpers::TopLevelAccelerationStructure& topLevelAccelerationStructure, const Constants& constants)
    {
        if (!topLevelAccelerationStructure.Valid) throw std::invalid_argument("top-level acceleration structure has not been built");
        PtContext* c = commandList.Context;
        ThrowIfFailed(c, pt_set_scene_data(c, GPUBuffers.SceneData));
        ThrowIfFailed(c, pt_set_camera(c, GPUBuffers.Camera));
        ThrowIfFailed(c, pt_set_instance_data(c, GPUBuffers.InstanceData, GPUBuffers.InstanceCount));
        ThrowIfFailed(c, pt_set_object_data(c, GPUBuffers.ObjectData, GPUBuffers.ObjectCount));
        PtGBufferConstants k{ { constants.RenderSize[0], constants.RenderSize[1] }, constants.Flags };
        ThrowIfFailed(c, pt_gbuffer_render(c, &k, &Textures));
    }

private:
    PtContext* m_context;
};

// struct SHARC, Source/SHARC.ixx: the radiance cache's buffers (context-owned here) and its constants
struct SHARC {
    struct ConstantsData { uint32_t AccumulationFrames = 10, MaxStaleFrames = 64; float SceneScale = 50; bool IsAntiFireflyEnabled = true; };

    explicit SHARC(CommandList& commandList) : m_context(commandList.Context) {}
    void Configure(uint32_t capacity = 1u << 22) { ThrowIfFailed(m_context, pt_sharc_configure(m_context, capacity)); }   // a multiple of 32; empties the cache
    void Reset() { ThrowIfFailed(m_context, pt_sharc_reset(m_context)); }                                                   // App.cpp:682-685
    uint32_t LiveEntries() { uint32_t n = 0; ThrowIfFailed(m_context, pt_sharc_download(m_context, nullptr, 0, &n)); return n; }
    ConstantsData Constants{};

private:
    PtContext* m_context;
};

struct Raytracing {
    struct SHARCSettings { uint32_t DownscaleFactor = 4; float RoughnessThreshold = 0.4f; bool IsHashGridVisualizationEnabled = false; };   // Source/Raytracing.ixx, MyAppData.h:250-262
    struct GraphicsSettings {                               // Source/Raytracing.ixx:30-36
        uint32_t RenderSize[2]{};
        uint32_t FrameIndex{}, Bounces{}, SamplesPerPixel{};
        float ThroughputThreshold = 1e-3f;
        bool IsRussianRouletteEnabled{}, IsShaderExecutionReorderingEnabled{}, IsDIEnabled{};
        uint32_t Denoiser{};
    };

    struct { const PtSceneData* SceneData; const PtCamera* Camera; const PtObjectData* ObjectData; uint32_t ObjectCount; } GPUBuffers{};
    PtTextures Textures{};                                  // Position .. Radiance; Diffuse / Specular / SpecularHitDistance when GraphicsSettings.Denoiser != None

    explicit Raytracing(CommandList& commandList) : m_context(commandList.Context) {}

    void SetConstants(const GraphicsSettings& graphicsSettings) noexcept      // Source/Raytracing.ixx:92-104
    {
        m_graphicsSettings = {};
        m_graphicsSettings.RenderSize[0] = graphicsSettings.RenderSize[0];
        m_graphicsSettings.RenderSize[1] = graphicsSettings.RenderSize[1];
        m_graphicsSettings.FrameIndex = graphicsSettings.FrameIndex;
        m_graphicsSettings.Bounces = graphicsSettings.Bounces;
        m_graphicsSettings.SamplesPerPixel = graphicsSettings.SamplesPerPixel;
        m_graphicsSettings.ThroughputThreshold = graphicsSettings.ThroughputThreshold;
        m_graphicsSettings.IsRussianRouletteEnabled = graphicsSettings.IsRussianRouletteEnabled;
        m_graphicsSettings.IsShaderExecutionReorderingEnabled = graphicsSettings.IsShaderExecutionReorderingEnabled;
        m_graphicsSettings.IsDIEnabled = graphicsSettings.IsDIEnabled;
        m_graphicsSettings.Denoiser = graphicsSettings.Denoiser;
    }

    void Render(CommandList& commandList, const RaytracingHelpers::TopLevelAccelerationStructure& topLevelAccelerationStructure)   // :106-112
    {
        if (!topLevelAccelerationStructure.Valid) throw std::invalid_argument("top-level acceleration structure has not been built");
        PtContext* c = commandList.Context;
        ThrowIfFailed(c, pt_set_scene_data(c, GPUBuffers.SceneData));
        ThrowIfFailed(c, pt_set_camera(c, GPUBuffers.Camera));
        ThrowIfFailed(c, pt_set_object_data(c, GPUBuffers.ObjectData, GPUBuffers.ObjectCount));
        ThrowIfFailed(c, pt_raytrace_set_constants(c, &m_graphicsSettings));
        ThrowIfFailed(c, pt_raytrace_render(c, &Textures));
    }

    // the overload with RTXGITechnique::SHARC (:114-148): clear, update, resolve, query, swap
    void Render(CommandList& commandList, const RaytracingHelpers::TopLevelAccelerationStructure& topLevelAccelerationStructure, SHARC& sharc, const SHARCSettings& sharcSettings)
    {
        if (!topLevelAccelerationStructure.Valid) throw std::invalid_argument("top-level acceleration structure has not been built");
        PtContext* c = commandList.Context;
        PtSHARCSettings s{};
        s.AccumulationFrames = sharc.Constants.AccumulationFrames; s.MaxStaleFrames = sharc.Constants.MaxStaleFrames; s.SceneScale = sharc.Constants.SceneScale;
        s.IsAntiFireflyEnabled = sharc.Constants.IsAntiFireflyEnabled; s.DownscaleFactor = sharcSettings.DownscaleFactor;
        s.RoughnessThreshold = sharcSettings.RoughnessThreshold; s.IsHashGridVisualizationEnabled = sharcSettings.IsHashGridVisualizationEnabled;
        ThrowIfFailed(c, pt_set_scene_data(c, GPUBuffers.SceneData));
        ThrowIfFailed(c, pt_set_camera(c, GPUBuffers.Camera));
        ThrowIfFailed(c, pt_set_object_data(c, GPUBuffers.ObjectData, GPUBuffers.ObjectCount));
        ThrowIfFailed(c, pt_raytrace_set_constants(c, &m_graphicsSettings));
        ThrowIfFailed(c, pt_sharc_set_constants(c, &s));
        ThrowIfFailed(c, pt_raytrace_render_sharc(c, &Textures));
    }

private:
    PtContext* m_context;
    PtGraphicsSettings m_graphicsSettings{};
};

// App::PostProcessGraphics with Denoiser::None (Source/App.cpp:1506-1571): Bloom + Merge (ProcessBloom :1769-1775), DirectXTK's
// ToneMapPostProcess (ToneMap :1777-1803) and the copy into the R10G10B10A2_UNORM back buffer (CopyTexture :1805-1812), enqueued after
// Raytracing::Render. The settings carry the names of MyAppData::Settings::Graphics::PostProcessing (Source/MyAppData.h:305-333). Runs on
// the full frame: a sharded host calls it on rank 0 after the gather.
struct PostProcessing {
    enum class ToneMapOperator : uint32_t { Saturate = PT_TONE_MAP_SATURATE, Reinhard = PT_TONE_MAP_REINHARD, ACESFilmic = PT_TONE_MAP_ACES_FILMIC };
    enum class ColorRotation : uint32_t {
        HDTVtoUHDTV = PT_COLOR_ROTATION_HDTV_TO_UHDTV, DCI_P3_D65toUHDTV = PT_COLOR_ROTATION_DCI_P3_D65_TO_UHDTV,
        HDTVtoDCI_P3_D65 = PT_COLOR_ROTATION_HDTV_TO_DCI_P3_D65
    };
    struct Settings {
        uint32_t RenderSize[2]{};
        struct { bool IsEnabled = true; float Strength = 0.05f; } Bloom;                               // [0, 1]
        struct {
            struct { float PaperWhiteNits = 200; ColorRotation ColorPrimaryRotation = ColorRotation::HDTVtoUHDTV; } HDR;   // [50, 10000]
            struct { ToneMapOperator Operator = ToneMapOperator::ACESFilmic; float Exposure = 0; } NonHDR;                   // [-10, 10]
        } ToneMapping;
        bool IsHDREnabled = false;                                     // the reference asks the display; this library has none
    };

    PtPostTextures Textures{};                              // Radiance in; Color, BackBuffer, Display8 out (NULL: not written)

    explicit PostProcessing(CommandList& commandList) : m_context(commandList.Context) {}

    void SetConstants(const Settings& settings)
    {
        PtPostProcessSettings s{};
        s.RenderSize[0] = settings.RenderSize[0]; s.RenderSize[1] = settings.RenderSize[1];
        s.IsBloomEnabled = settings.Bloom.IsEnabled; s.BloomStrength = settings.Bloom.Strength;
        s.IsHDREnabled = settings.IsHDREnabled;
        s.ToneMappingOperator = (uint32_t)settings.ToneMapping.NonHDR.Operator; s.Exposure = settings.ToneMapping.NonHDR.Exposure;
        s.PaperWhiteNits = settings.ToneMapping.HDR.PaperWhiteNits; s.ColorPrimaryRotation = (uint32_t)settings.ToneMapping.HDR.ColorPrimaryRotation;
        ThrowIfFailed(m_context, pt_post_set_constants(m_context, &s));
    }

    void Render(CommandList& commandList) { ThrowIfFailed(commandList.Context, pt_post_render(commandList.Context, &Textures)); }

private:
    PtContext* m_context;
};

// struct NRDComposition (Source/NRDComposition.ixx -> Shaders/NRDComposition.hlsl:36-88): the pass App::ProcessNRD (Source/App.cpp:1595-1688)
// runs in front of the denoiser (IsPack: Diffuse / Specular become its input encoding, in place) and behind it (the denoised pair is unpacked,
// multiplied by the albedos and added to Radiance). The denoiser between the two calls is the host's. Element-wise: a sharded host passes its
// own rows and their size. DenoisedDiffuse / DenoisedSpecular may be NoisyDiffuse / NoisySpecular themselves (the identity denoiser).
struct NRDComposition {
    struct Constants {
        uint32_t RenderSize[2]{};
        bool IsPack{};
        uint32_t Denoiser{};                                  // PtDenoiser
        float ReBLURHitDistance[4]{};                         // nrd::ReblurSettings().hitDistanceParameters

        Constants() { pt_nrd_reblur_hit_distance_defaults(ReBLURHitDistance); }
    };

    PtNRDCompositionTextures Textures{};

    explicit NRDComposition(CommandList&) {}

    void Process(CommandList& commandList, const Constants& constants)
    {
        PtNRDCompositionConstants k{};
        k.RenderSize[0] = constants.RenderSize[0]; k.RenderSize[1] = constants.RenderSize[1];
        k.IsPack = constants.IsPack; k.Denoiser = constants.Denoiser;
        for (int i = 0; i < 4; i++) k.ReBLURHitDistance[i] = constants.ReBLURHitDistance[i];
        ThrowIfFailed(commandList.Context, pt_nrd_composition_process(commandList.Context, &k, &Textures));
    }
};

// The library's own denoiser for the ReLAX slot between the two calls of NRDComposition (pt_denoiser_*; DESIGN.md section 1, "Denoiser"):
// temporal accumulation with reprojection, a variance estimate, an edge-stopping a-trous wavelet. Not NRD's ReLAX, and ReLAX's packing
// only: SetConstants refuses Settings::Denoiser = PT_DENOISER_NRD_REBLUR. In App::ProcessNRD it stands where NRD::Denoise does. The
// Denoised pair may be the Noisy pair. Runs on the full frame: a sharded host calls it on the gathered textures.
struct Denoiser {
    struct Settings {
        uint32_t RenderSize[2]{};
        uint32_t MaxAccumulatedFrames = 30, AtrousIterations = 5;           // 1..255 | 0..8
        float DepthThreshold = 0.01f, NormalCosine = 0.8f;                  // (0, 1] | [0, 1)
        float DiffuseLuminanceSigma = 2, SpecularLuminanceSigma = 1, RoughnessFraction = 0.15f;   // > 0
        uint32_t Denoiser = PT_DENOISER_NRD_RELAX;                          // the packing of the pair it will be handed
    };

    PtDenoiserTextures Textures{};

    explicit Denoiser(CommandList& commandList) : m_context(commandList.Context) {}

    void SetConstants(const Settings& settings)
    {
        if (settings.Denoiser != PT_DENOISER_NRD_RELAX)
            throw std::invalid_argument("the denoiser reads ReLAX's packing (radiance, hit distance) only: ReBLUR's (YCoCg, normalised hit distance) "
                                        "and the other Denoiser values are not served");
        PtDenoiserSettings s{};
        s.RenderSize[0] = settings.RenderSize[0]; s.RenderSize[1] = settings.RenderSize[1];
        s.MaxAccumulatedFrames = settings.MaxAccumulatedFrames; s.AtrousIterations = settings.AtrousIterations;
        s.DepthThreshold = settings.DepthThreshold; s.NormalCosine = settings.NormalCosine;
        s.DiffuseLuminanceSigma = settings.DiffuseLuminanceSigma; s.SpecularLuminanceSigma = settings.SpecularLuminanceSigma;
        s.RoughnessFraction = settings.RoughnessFraction;
        ThrowIfFailed(m_context, pt_denoiser_set_constants(m_context, &s));
    }

    void Process(CommandList& commandList) { ThrowIfFailed(commandList.Context, pt_denoiser_process(commandList.Context, &Textures)); }

    void ResetHistory() { ThrowIfFailed(m_context, pt_denoiser_reset_history(m_context)); }

    // the accumulated length of the diffuse channel per pixel after the last Process, row-major; empty when there is no history. Synchronises.
    std::vector<float> DownloadHistory(uint32_t& width, uint32_t& height)
    {
        ThrowIfFailed(m_context, pt_denoiser_download_history(m_context, nullptr, 0, &width, &height));
        std::vector<float> out((size_t)width * height);
        if (!out.empty()) ThrowIfFailed(m_context, pt_denoiser_download_history(m_context, out.data(), out.size(), &width, &height));
        return out;
    }

private:
    PtContext* m_context;
};

// The library's own temporal upscaler for the super-resolution step of App::PostProcessGraphics (Source/App.cpp:1532-1541), between the
// denoiser and Bloom / ToneMap, where the reference calls DLSS or XeSS (pt_upscaler_*; DESIGN.md section 1, "Upscaler"): a temporal
// accumulating upscaler from RenderSize to OutputSize. Not a port of either SDK. Process takes the Camera.Jitter the frame was rendered
// with (as it stands in PtCamera); Color then is the post chain's Radiance. Runs on the full frame of an unsharded context.
struct Upscaler {
    using SuperResolutionMode = PtSuperResolutionMode;                     // Source/Upscaler.ixx

    struct Settings {
        uint32_t RenderSize[2]{}, OutputSize[2]{};                          // RenderSize <= OutputSize <= 4 RenderSize per axis
        uint32_t MaxAccumulatedFrames = 16;                                 // 1..255
        float KernelRadius = 1, DepthThreshold = 0.01f;                     // [0.75, 2] | (0, 1]
    };

    PtUpscalerTextures Textures{};

    explicit Upscaler(CommandList& commandList) : m_context(commandList.Context) {}

    void SetConstants(const Settings& settings)
    {
        PtUpscalerSettings s{};
        s.RenderSize[0] = settings.RenderSize[0]; s.RenderSize[1] = settings.RenderSize[1];
        s.OutputSize[0] = settings.OutputSize[0]; s.OutputSize[1] = settings.OutputSize[1];
        s.MaxAccumulatedFrames = settings.MaxAccumulatedFrames; s.KernelRadius = settings.KernelRadius; s.DepthThreshold = settings.DepthThreshold;
        ThrowIfFailed(m_context, pt_upscaler_set_constants(m_context, &s));
    }

    void Process(CommandList& commandList, const float (&jitter)[2]) { ThrowIfFailed(commandList.Context, pt_upscaler_process(commandList.Context, &Textures, jitter)); }

    void ResetHistory() { ThrowIfFailed(m_context, pt_upscaler_reset_history(m_context)); }

    // the accumulated weight n per output pixel after the last Process, row-major; empty when there is no history. Synchronises.
    std::vector<float> DownloadHistory(uint32_t& width, uint32_t& height)
    {
        ThrowIfFailed(m_context, pt_upscaler_download_history(m_context, nullptr, 0, &width, &height));
        std::vector<float> out((size_t)width * height);
        if (!out.empty()) ThrowIfFailed(m_context, pt_upscaler_download_history(m_context, out.data(), out.size(), &width, &height));
        return out;
    }

    // host only: the render size of a mode for an output size, and the Camera.Jitter of a frame
    static void RenderSize(SuperResolutionMode mode, const uint32_t (&output)[2], uint32_t (&render)[2])
    {
        if (pt_upscaler_render_size((uint32_t)mode, output, render) != PT_OK) throw std::invalid_argument("Upscaler::RenderSize: a mode or an output size out of range");
    }
    static void Jitter(uint64_t frameIndex, const uint32_t (&render)[2], const uint32_t (&output)[2], float (&jitter)[2])
    {
        if (pt_upscaler_jitter(frameIndex, render, output, jitter) != PT_OK) throw std::invalid_argument("Upscaler::Jitter: a size out of range");
    }

private:
    PtContext* m_context;
};

// The library's own denoising upscaler for the ray-reconstruction step of App::PostProcessGraphics (Source/App.cpp:1513-1523), where the
// reference's default settings call ProcessDLSSRayReconstruction (pt_reconstruction_*; DESIGN.md section 1, "Ray reconstruction"): from
// the noisy Radiance of a Denoiser = DLSSRayReconstruction frame, the two albedos and the G-buffer guides at RenderSize to the denoised
// Color at OutputSize. Not a port of the SDK. Process takes the Camera.Jitter the frame was rendered with (Upscaler::RenderSize and
// Upscaler::Jitter serve this pass too); Color then is the post chain's Radiance. Runs on the full frame of an unsharded context.
struct Reconstruction {
    struct Settings {
        uint32_t RenderSize[2]{}, OutputSize[2]{};                          // RenderSize <= OutputSize <= 4 RenderSize per axis
        uint32_t MaxAccumulatedFrames = 30, MaxOutputFrames = 16;           // 1..255: the history at RenderSize | at OutputSize
        uint32_t AtrousIterations = 5;                                      // 0..8
        float DepthThreshold = 0.01f, NormalCosine = 0.8f;                  // (0, 1] | [0, 1)
        float LuminanceSigma = 2, RoughnessFraction = 0.15f, KernelRadius = 1;   // > 0 | > 0 | [0.75, 2]
    };

    PtReconstructionTextures Textures{};

    explicit Reconstruction(CommandList& commandList) : m_context(commandList.Context) {}

    void SetConstants(const Settings& settings)
    {
        PtReconstructionSettings s{};
        s.RenderSize[0] = settings.RenderSize[0]; s.RenderSize[1] = settings.RenderSize[1];
        s.OutputSize[0] = settings.OutputSize[0]; s.OutputSize[1] = settings.OutputSize[1];
        s.MaxAccumulatedFrames = settings.MaxAccumulatedFrames; s.MaxOutputFrames = settings.MaxOutputFrames; s.AtrousIterations = settings.AtrousIterations;
        s.DepthThreshold = settings.DepthThreshold; s.NormalCosine = settings.NormalCosine; s.LuminanceSigma = settings.LuminanceSigma;
        s.RoughnessFraction = settings.RoughnessFraction; s.KernelRadius = settings.KernelRadius;
        ThrowIfFailed(m_context, pt_reconstruction_set_constants(m_context, &s));
    }

    void Process(CommandList& commandList, const float (&jitter)[2]) { ThrowIfFailed(commandList.Context, pt_reconstruction_process(commandList.Context, &Textures, jitter)); }

    void ResetHistory() { ThrowIfFailed(m_context, pt_reconstruction_reset_history(m_context)); }

    // after the last Process, row-major: the history length of the signal per render pixel and the accumulated weight n per output pixel;
    // both empty when there is no history. Synchronises.
    void DownloadHistory(std::vector<float>& length, uint32_t (&render)[2], std::vector<float>& n, uint32_t (&output)[2])
    {
        ThrowIfFailed(m_context, pt_reconstruction_download_history(m_context, nullptr, nullptr, 0, nullptr, 0, render, output));
        length.assign((size_t)render[0] * render[1], 0.0f); n.assign((size_t)output[0] * output[1], 0.0f);
        if (!length.empty())
            ThrowIfFailed(m_context, pt_reconstruction_download_history(m_context, length.data(), nullptr, length.size(), n.data(), n.size(), render, output));
    }

private:
    PtContext* m_context;
};

// The library's own frame interpolator for the frame-generation step of App::PostProcessGraphics (Source/App.cpp:1564-1566), behind
// ToneMap, where the reference's default settings hand DLSS-G the depth, the motion vectors and the HUD-less colour
// (pt_frame_generation_*; DESIGN.md section 1, "Frame generation"): from the tone-mapped Color of this frame and of the one before it to
// the frame at Phase between them. Not a port of DLSS-G or FSR 3, and unpinned against both. Process takes the Camera.Jitter the frame
// was rendered with and returns whether Generated is an interpolated frame (false on the call without a previous frame: Generated is
// Color). A host displays Generated, then Color. Runs on the full frame of an unsharded context.
static_assert(sizeof(PtFrameGenerationSettings) == 48, "PtFrameGenerationSettings is 48 B");
struct FrameGeneration {
    struct Settings {
        uint32_t RenderSize[2]{}, OutputSize[2]{};                          // RenderSize <= OutputSize <= 4 RenderSize per axis
        float Phase = 0.5f, DepthThreshold = 0.01f;                         // (0, 1) | (0, 1]
    };

    PtFrameGenerationTextures Textures{};

    explicit FrameGeneration(CommandList& commandList) : m_context(commandList.Context) {}

    void SetConstants(const Settings& settings)
    {
        PtFrameGenerationSettings s{};
        s.RenderSize[0] = settings.RenderSize[0]; s.RenderSize[1] = settings.RenderSize[1];
        s.OutputSize[0] = settings.OutputSize[0]; s.OutputSize[1] = settings.OutputSize[1];
        s.Phase = settings.Phase; s.DepthThreshold = settings.DepthThreshold;
        ThrowIfFailed(m_context, pt_frame_generation_set_constants(m_context, &s));
    }

    bool Process(CommandList& commandList, const float (&jitter)[2])
    {
        uint32_t generated = 0;
        ThrowIfFailed(commandList.Context, pt_frame_generation_process(commandList.Context, &Textures, jitter, &generated));
        return generated != 0;
    }

    void ResetHistory() { ThrowIfFailed(m_context, pt_frame_generation_reset_history(m_context)); }

    // after the last Process that generated a frame, row-major: the midpoint field per render pixel and the PtFrameGenerationClass byte per
    // output pixel; both empty when the last call generated nothing. Synchronises.
    void DownloadField(std::vector<uint64_t>& field, uint32_t (&render)[2], std::vector<uint8_t>& classes, uint32_t (&output)[2])
    {
        ThrowIfFailed(m_context, pt_frame_generation_download_field(m_context, nullptr, 0, nullptr, 0, render, output));
        field.assign((size_t)render[0] * render[1], 0); classes.assign((size_t)output[0] * output[1], 0);
        if (!field.empty())
            ThrowIfFailed(m_context, pt_frame_generation_download_field(m_context, field.data(), field.size(), classes.data(), classes.size(), render, output));
    }

private:
    PtContext* m_context;
};

// The library's own edge-adaptive sharpening filter for the image-scaling step of App::PostProcessGraphics (App::ProcessNIS,
// Source/App.cpp:1544-1548, :1756-1766), between the upscaler and Bloom, where the reference runs NVIDIA Image Scaling in its sharpen mode
// with NIS.Sharpness (pt_sharpen_*; DESIGN.md section 1, "Sharpening"): from the linear HDR Color the post chain would read to Sharpened,
// which the post chain then reads. Not a port of NVIDIA Image Scaling, and unpinned against it. No history and no memory of its own; a
// sharded host runs it on the gathered frame.
static_assert(sizeof(PtSharpenSettings) == 32, "PtSharpenSettings is 32 B");
struct Sharpening {
    struct Settings {
        uint32_t Size[2]{};                                                 // the size the post chain runs at
        float Sharpness = 0.5f, ContrastFloor = 0.015625f;                  // [0, 1] (NIS.Sharpness) | [2^-10, 0.5]
    };

    PtSharpenTextures Textures{};

    explicit Sharpening(CommandList& commandList) : m_context(commandList.Context) {}

    void SetConstants(const Settings& settings)
    {
        PtSharpenSettings s{};
        s.Size[0] = settings.Size[0]; s.Size[1] = settings.Size[1];
        s.Sharpness = settings.Sharpness; s.ContrastFloor = settings.ContrastFloor;
        ThrowIfFailed(m_context, pt_sharpen_set_constants(m_context, &s));
    }

    void Process(CommandList& commandList) { ThrowIfFailed(commandList.Context, pt_sharpen_process(commandList.Context, &Textures)); }

private:
    PtContext* m_context;
};

// struct MipmapGeneration (Source/MipmapGeneration.ixx: SetTexture + Process) for an R32_FLOAT texture: Process reads level 0 and writes the
// other levels of the chain (pt_mipmap_generate). App::PrepareReSTIRDI (Source/App.cpp:1095-1116) runs it on the LocalLightPDF texture; the DI
// pass here does that itself (DirectLighting::SetPdfMipmap), so a host needs this operator only for a texture of its own.
struct MipmapGeneration {
    explicit MipmapGeneration(CommandList&) {}

    // levels[k]: the device memory of level k, row-major, max(1, width >> k) x max(1, height >> k) floats
    void SetTexture(std::vector<float*> levels, uint32_t width, uint32_t height)
    {
        m_levels = std::move(levels); m_width = width; m_height = height;
    }

    void Process(CommandList& commandList)
    {
        ThrowIfFailed(commandList.Context, pt_mipmap_generate(commandList.Context, m_levels.empty() ? nullptr : m_levels.data(), m_width, m_height, (uint32_t)m_levels.size()));
    }

private:
    std::vector<float*> m_levels;
    uint32_t m_width = 0, m_height = 0;
};

} // namespace ptamd
