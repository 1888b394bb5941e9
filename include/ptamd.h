/*
 * ptamd.h -- C ABI of the MI355X-native wavefront path tracer (libptamd.so).
 *
 * Drop-in boundary for ONE hot path of Hydr10n/DirectX-Physically-Based-Raytracer:
 *     GBufferGeneration::Render  (Source/GBufferGeneration.ixx:80-117 -> Shaders/GBufferGeneration.hlsl:116-232)
 *     Raytracing::Render         (Source/Raytracing.ixx:106-112      -> Shaders/Raytracing.hlsl:103-415, DEFAULT)
 *     acceleration-structure build (Source/Scene.ixx:286-380, Source/RaytracingHelpers.ixx:28-105,
 *                                   Source/CommandList.ixx:217-249)
 * Every entry point cites the reference interface it replaces. Plain pointers and sizes only:
 * no C++ types, no torch types. All `const void*` "device" arguments are HIP device pointers
 * owned by the caller; structs passed by pointer are HOST memory copied during the call.
 * Work is enqueued on the context's HIP stream (pt_set_stream) and is asynchronous unless
 * stated otherwise; pt_sync() blocks until it has completed.
 *
 * Error convention: every function returns PT_OK (0) or a negative PtStatus; the message is
 * available from pt_last_error(). Nothing throws across this boundary. (The reference throws
 * std::system_error / std::invalid_argument: Source/ErrorHelpers.ixx:16-32,
 * Source/RaytracingHelpers.ixx:83-88 -- the C++ mirror in directx-physically-based-raytracer_amd/host/
 * turns the status back into those exceptions.)
 */
#ifndef PTAMD_H
#define PTAMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PTAMD_ABI_VERSION 4

typedef enum PtStatus {
    PT_OK = 0,
    PT_ERROR_INVALID_ARGUMENT = -1,   /* reference: Throw<std::invalid_argument> */
    PT_ERROR_HIP = -2,                /* reference: ThrowIfFailed(HRESULT) */
    PT_ERROR_OUT_OF_MEMORY = -3,
    PT_ERROR_NOT_READY = -4,          /* render before an acceleration structure exists */
    PT_ERROR_NO_DEVICE = -5,
    PT_ERROR_RCCL = -6                /* an RCCL call failed (message: ncclGetErrorString), or librccl could not be loaded */
} PtStatus;

/* ------------------------------------------------------------------------------------------
 * Reference data layouts, byte-exact. Field names are the reference's.
 * ------------------------------------------------------------------------------------------ */
typedef struct PtVertexDesc {             /* Source/Vertex.ixx:30-36, Shaders/Vertex.hlsli:5-12 */
    uint32_t Stride, _pad[3];
    struct { uint32_t Normal, Tangent, TextureCoordinates[2]; } AttributeOffsets;   /* ~0u = absent */
} PtVertexDesc;

typedef struct PtMeshDescriptors {        /* Source/CommonShaderData.ixx:28-30; indices into the descriptor heap */
    uint32_t Vertices, Indices, MotionVectors, _pad;
} PtMeshDescriptors;

typedef struct PtMaterial {               /* Source/Material.ixx:12-20, Shaders/Material.hlsli:8-22 */
    float BaseColor[4];
    float EmissiveStrength;
    float EmissiveColor[3];
    float Metallic, Roughness, IOR, Transmission;
    uint32_t AlphaMode;                   /* 0 Opaque, 1 Mask, 2 Blend */
    float AlphaCutoff;
    uint32_t _pad[2];
} PtMaterial;

typedef struct PtTextureMapInfo {         /* Source/Material.ixx:35-38 */
    uint32_t Descriptor, TextureCoordinateIndex, _pad[2];
} PtTextureMapInfo;

typedef struct PtObjectData {             /* Source/CommonShaderData.ixx:34-39 */
    PtVertexDesc VertexDesc;
    PtMeshDescriptors MeshDescriptors;
    PtMaterial Material;
    PtTextureMapInfo TextureMapInfoArray[7];
} PtObjectData;

typedef struct PtInstanceData {           /* Source/CommonShaderData.ixx:22-26 */
    uint32_t FirstGeometryIndex, _pad[3];
    float PreviousObjectToWorld[12];      /* XMFLOAT3X4: rows of the column-vector affine [R|t] */
    float ObjectToWorld[12];
} PtInstanceData;

typedef struct PtSceneData {              /* Source/CommonShaderData.ixx:15-20 */
    uint32_t IsStatic, IsEnvironmentLightTextureCubeMap;
    uint32_t EnvironmentLightTextureDescriptor, _pad;
    float EnvironmentLightColor[4];       /* a < 0 selects the procedural sky (Shaders/ShadingHelpers.hlsli:25-29) */
    float EnvironmentLightTransform[12];
} PtSceneData;

typedef struct PtCamera {                 /* Source/Camera.ixx:16-36, Shaders/Camera.hlsli:5-25 */
    uint32_t IsNormalizedDepthReversed;
    float PreviousPosition[3], Position[3], _pad0;
    float RightDirection[3], _pad1;
    float UpDirection[3], _pad2;
    float ForwardDirection[3];
    float ApertureRadius, NearDepth, FarDepth;
    float Jitter[2];
    float PreviousWorldToView[16], PreviousViewToProjection[16], PreviousWorldToProjection[16],
          PreviousProjectionToView[16], PreviousViewToWorld[16], WorldToProjection[16],
          ProjectionToView[16], ViewToWorld[16];
} PtCamera;

typedef struct PtGraphicsSettings {       /* Raytracing::GraphicsSettings, Source/Raytracing.ixx:30-36,151-166 */
    uint32_t RenderSize[2];
    uint32_t FrameIndex, Bounces, SamplesPerPixel;
    float ThroughputThreshold;            /* reference default 1e-3 */
    uint32_t IsRussianRouletteEnabled, IsShaderExecutionReorderingEnabled, IsDIEnabled;
    uint32_t Denoiser;                    /* PtDenoiser: selects which outputs Raytracing writes (Raytracing.hlsl:379-413) */
    uint32_t ExtFlags;                    /* reference: first padding word. PT_EXT_* build-side switches */
    uint32_t _pad;
    uint32_t SHARC[8];                    /* ignored: the radiance cache has calls of its own (pt_sharc_*, below) */
} PtGraphicsSettings;

/* enum class Denoiser, Source/Denoiser.ixx:8. The denoisers themselves (NRD, DLSS-RR) are out of scope; these values only
 * select the output packing the path tracer hands to them. */
enum PtDenoiser { PT_DENOISER_NONE = 0, PT_DENOISER_DLSS_RAY_RECONSTRUCTION = 1, PT_DENOISER_NRD_REBLUR = 2, PT_DENOISER_NRD_RELAX = 3 };

#define PT_EXT_LAMBERTIAN_ONLY 0x1u       /* BASELINE.json config C1: lobe weights {1,0,0}, DiffuseTerm = 1/pi */

typedef struct PtGBufferConstants {       /* GBufferGeneration::Constants, Source/GBufferGeneration.ixx:46-49 */
    uint32_t RenderSize[2];
    uint32_t Flags;                       /* PtGBufferFlags */
} PtGBufferConstants;

enum PtGBufferFlags {                     /* Source/GBufferGeneration.ixx:28-44 */
    PT_GB_Position = 0x1, PT_GB_FlatNormal = 0x2, PT_GB_GeometricNormal = 0x4, PT_GB_LinearDepth = 0x8,
    PT_GB_NormalizedDepth = 0x10, PT_GB_MotionVector = 0x20, PT_GB_DiffuseAlbedo = 0x40,
    PT_GB_SpecularAlbedo = 0x80, PT_GB_Albedo = 0xC0, PT_GB_NormalRoughness = 0x100, PT_GB_Radiance = 0x200,
    PT_GB_Geometry = 0x1 | 0x2 | 0x4 | 0x8 | 0x10 | 0x20 | 0x100,
    PT_GB_Material = 0x400 | 0xC0 | 0x100 | 0x200
};

/* The G-buffer "textures": linear row-major device arrays, one element per pixel of the LOCAL
 * framebuffer (see PtSharding), in the reference's DXGI formats (Source/App.cpp:438-455).
 * Same member order as GBufferGeneration::Textures (Source/GBufferGeneration.ixx:53-68);
 * Raytracing::Textures (Source/Raytracing.ixx:46-59) is the subset the path tracer reads plus
 * Radiance. NULL = not bound. DiffuseAlbedo / SpecularAlbedo (GBufferGeneration.hlsl:171-186) are written only when
 * their flag is set, which the reference does when a denoiser is selected (Source/App.cpp:1223). */
typedef struct PtTextures {
    void* Position;            /* R32G32B32A32_FLOAT  16 B : xyz world position, w = spawn offset; all +inf on miss */
    void* FlatNormal;          /* R16G16_SNORM         4 B : signed octahedral */
    void* GeometricNormal;     /* R16G16_SNORM         4 B */
    void* LinearDepth;         /* R32_FLOAT            4 B */
    void* NormalizedDepth;     /* R32_FLOAT            4 B */
    void* MotionVector;        /* R16G16B16A16_FLOAT   8 B */
    void* BaseColorMetalness;  /* R8G8B8A8_UNORM       4 B */
    void* DiffuseAlbedo;       /* R16G16B16A16_FLOAT   8 B  NRD_MaterialFactors diffuse (only with PT_GB_DiffuseAlbedo) */
    void* SpecularAlbedo;      /* R16G16B16A16_FLOAT   8 B  NRD_MaterialFactors specular (only with PT_GB_SpecularAlbedo) */
    void* NormalRoughness;     /* R16G16B16A16_SNORM   8 B */
    void* IOR;                 /* R16_FLOAT            2 B */
    void* Transmission;        /* R8_UNORM             1 B */
    void* Radiance;            /* R16G16B16A16_FLOAT   8 B : G-buffer emission/environment in, path-traced radiance out */
    void* RadianceF32;         /* build-side extra, optional: R32G32B32A32_FLOAT copy of the value stored to Radiance */
    /* denoiser-facing outputs of Raytracing::Textures (Source/Raytracing.ixx:55-58), written per Raytracing.hlsl:387-413 */
    void* Diffuse;             /* R16G16B16A16_FLOAT   8 B : NRD: indirect diffuse radiance, hit distance in a */
    void* Specular;            /* R16G16B16A16_FLOAT   8 B : NRD: indirect specular radiance, hit distance in a */
    void* SpecularHitDistance; /* R16_FLOAT            2 B : DLSS-RR: first-bounce hit distance of specular pixels */
} PtTextures;

/* ------------------------------------------------------------------------------------------
 * context
 * ------------------------------------------------------------------------------------------ */
typedef struct PtContext PtContext;

int  pt_abi_version(void);
/* One context per GPU (reference: one D3D12 device, Source/DeviceResources.cpp:101-170). */
int  pt_create(int device_ordinal, PtContext** out_ctx);
void pt_destroy(PtContext* ctx);
const char* pt_last_error(const PtContext* ctx);            /* ctx may be NULL: last error of pt_create */
/* hipStream_t to enqueue on (NULL = the default stream). Reference: CommandList recording order. */
int  pt_set_stream(PtContext* ctx, void* hip_stream);
int  pt_sync(PtContext* ctx);                               /* reference: CommandList::End/Wait, Source/CommandList.ixx:86-119 */
/* How many contexts render concurrently on this GPU (frames in flight on separate streams; reference: the swap chain's
 * back-buffer count, Source/DeviceResources.cpp). A performance hint only -- it sizes the persistent grids: a kernel that shares
 * the GPU with other frames' kernels launches fewer, longer-lived workgroups. Default 1. */
int  pt_set_frames_in_flight(PtContext* ctx, uint32_t frames);
/* Chains of a frame. Paths never leave their sub-queue of the path queue, so after the first bounce the rounds of a group of sub-queues depend
 * on nothing outside the group: the library runs `chains` such groups as independent chains of launches, each on a stream of its own (forked
 * from and joined to the context's stream, invisible to the caller), so that ONE frame's launches overlap the way frames in flight do -- for a
 * host that presents one frame at a time (the reference: Source/App.cpp:167). 0 = the library's choice: 3 for a scene beyond LDS rendered on a
 * caller-provided stream with pt_set_frames_in_flight(1), else 1 (measured: profiles/r04_ab/frame_chains.jsonl). On the default stream and while
 * kernel timing is enabled the chains run one after the other. The image does not depend on it. */
int  pt_set_round_chains(PtContext* ctx, uint32_t chains);            /* 0..4 */

/* ------------------------------------------------------------------------------------------
 * descriptor heap analogue. ObjectData.MeshDescriptors.{Vertices,Indices} index this table
 * (reference: ResourceDescriptorHeap[...], Shaders/RaytracingHelpers.hlsli:82-85).
 * stride: element size of a typed buffer (index buffer: 2 = R16_UINT or 4 = R32_UINT), 0 for raw (vertex) buffers,
 * 8 for the structured float16_t4 motion-vector buffer of a skinned mesh (MeshDescriptors.MotionVectors).
 * ------------------------------------------------------------------------------------------ */
int  pt_heap_resize(PtContext* ctx, uint32_t descriptor_count);
int  pt_heap_set_buffer(PtContext* ctx, uint32_t descriptor, const void* device_ptr, uint64_t bytes, uint32_t stride);
/* Texture2D / TextureCube SRV (reference: Texture::GetSRVDescriptor, indices stored in TextureMapInfo.Descriptor
 * at Source/App.cpp:1052-1063 and in SceneData.EnvironmentLightTextureDescriptor at :1021-1024). Mip 0 only: the
 * path samples with SampleLevel(sampler, uv, 0) (Shaders/ShadingHelpers.hlsli:58). Linear row-major texels;
 * a cube is 6 faces +X,-X,+Y,-Y,+Z,-Z back to back.
 * Block-compressed formats (the DDS assets the reference loads through DirectXTex, Source/TextureHelpers.ixx:65-78) are
 * sampled in place: width / height are texels (any value >= 1), the memory holds ceil(w/4) * ceil(h/4) blocks of 4x4
 * texels, row-major and tightly packed (D3D's mip 0 without row padding); texels of an edge block beyond the image are
 * never read. device_ptr must be aligned to the block size (8 / 16 bytes). 2D only: is_cube != 0 is refused. The decode
 * rules are DESIGN.md's ("Arithmetic spec"): a BC1 / BC3 texture samples to the bits of its RGBA8(_SRGB) expansion,
 * a BC4 / BC5 texture to the bits of its R32G32B32A32_FLOAT expansion. Values only grow; pt_abi_version() is unchanged. */
typedef enum PtFormat {
    PT_FORMAT_R8G8B8A8_UNORM = 0,
    PT_FORMAT_R8G8B8A8_UNORM_SRGB = 1,     /* base colour / emissive textures (Source/GLTFHelpers.ixx:375-391) */
    PT_FORMAT_R32G32B32A32_FLOAT = 2,      /* HDR environment maps */
    PT_FORMAT_BC1_UNORM = 3,               /*  8-byte blocks: rgb, a in {0, 1} (three-colour mode, index 3) */
    PT_FORMAT_BC1_UNORM_SRGB = 4,          /*  ... rgb through the sRGB table, a linear */
    PT_FORMAT_BC3_UNORM = 5,               /* 16-byte blocks: interpolated 8-bit alpha, then the BC1 colour half: rgba */
    PT_FORMAT_BC3_UNORM_SRGB = 6,          /*  ... rgb through the sRGB table, a linear */
    PT_FORMAT_BC4_UNORM = 7,               /*  8-byte blocks: (r, 0, 0, 1), the interpolants at fp32 precision */
    PT_FORMAT_BC5_UNORM = 8                /* 16-byte blocks: (r, g, 0, 1): two BC4 halves (normal maps) */
} PtFormat;
int  pt_heap_set_texture(PtContext* ctx, uint32_t descriptor, const void* device_ptr, uint32_t width, uint32_t height,
                         uint32_t format, uint32_t is_cube);

/* ------------------------------------------------------------------------------------------
 * acceleration structures
 * ------------------------------------------------------------------------------------------ */
typedef struct PtGeometryDesc {           /* D3D12_RAYTRACING_GEOMETRY_DESC as filled by CreateGeometryDesc,
                                             Source/RaytracingHelpers.ixx:76-105 */
    const void* VertexBuffer;             /* device; position = 3 x f32 at offset 0 of each vertex */
    uint32_t VertexCount, VertexStride;
    const void* IndexBuffer;              /* device */
    uint32_t IndexCount, IndexStride;     /* stride 2 or 4; count divisible by 3 (else PT_ERROR_INVALID_ARGUMENT) */
    uint32_t Flags;                       /* PT_GEOMETRY_FLAG_OPAQUE */
    uint32_t _pad;
} PtGeometryDesc;
#define PT_GEOMETRY_FLAG_OPAQUE 0x1u      /* Source/Scene.ixx:320-324 */

#define PT_BUILD_FLAG_ALLOW_UPDATE      0x01u
#define PT_BUILD_FLAG_PREFER_FAST_TRACE 0x04u
#define PT_BUILD_FLAG_PREFER_FAST_BUILD 0x08u

/* Bottom level: one per MeshNode, one geometry per Mesh (Source/Scene.ixx:286-341 ->
 * CommandList::BuildAccelerationStructures, Source/CommandList.ixx:217-233). Returns an id
 * (reference: RTXMU accel-struct id). A compressed 8-wide BVH is built on the device, on the context stream (Morton order,
 * binary hierarchy, surface-area-greedy collapse, 8-bit child boxes); the call returns when it is built. With
 * PT_BUILD_FLAG_ALLOW_UPDATE (the reference sets it for skeletal meshes, Scene.ixx:329) the structure keeps what a refit needs. */
int  pt_build_bottom_level(PtContext* ctx, const PtGeometryDesc* geometries, uint32_t geometry_count,
                           uint32_t build_flags, uint64_t* out_blas_id);
/* D3D12_RAYTRACING_ACCELERATION_STRUCTURE_BUILD_FLAG_PERFORM_UPDATE for a skinned mesh node (Source/Scene.ixx:327-341,
 * CommandList::UpdateAccelerationStructures, Source/CommandList.ixx:235-241): same id, geometry re-read from the (moved)
 * vertex buffers. A structure built with PT_BUILD_FLAG_ALLOW_UPDATE and given the same triangle counts is REFITTED in place
 * (asynchronous: no allocation, no wait); any other is rebuilt under its id. Until pt_build_top_level has been called again
 * (Scene::CreateAccelerationStructures does so every dynamic frame) renders answer PT_ERROR_NOT_READY. A rebuild whose tree would
 * take the live top level past the traversal stack's bound (2 * (top-level + deepest bottom-level depth) + 4 <= 64) is
 * PT_ERROR_INVALID_ARGUMENT and changes nothing: the old tree and the top level over it keep rendering. */
int  pt_update_bottom_level(PtContext* ctx, uint64_t blas_id, const PtGeometryDesc* geometries, uint32_t geometry_count, uint32_t build_flags);
/* Frees a bottom level. If the live top level refers to it, that top level is dropped with it (renders answer
 * PT_ERROR_NOT_READY until the next pt_build_top_level). */
int  pt_release_bottom_level(PtContext* ctx, uint64_t blas_id);

/* SkeletalMeshSkinning::Process (Source/SkeletalMeshSkinning.ixx:38-57 -> Shaders/SkeletalMeshSkinning.hlsl:28-62).
 * skeletal_vertices: VertexPositionNormalTangentSkin[vertex_count] (48 B); skeletal_transforms: row-major float3x4 per
 * joint; vertices: the mesh's 32-byte vertex buffer (read for the old position, rewritten); motion_vectors: half4 per
 * vertex (xyz written: old - new object-space position). All device pointers; enqueued on the stream. */
int  pt_skin_mesh(PtContext* ctx, const void* skeletal_vertices, const float* skeletal_transforms, void* vertices,
                  void* motion_vectors, uint32_t vertex_count);       /* Scene::CollectGarbage, Source/Scene.ixx:382-387 */

typedef struct PtInstanceDesc {           /* D3D12_RAYTRACING_INSTANCE_DESC as filled at Source/Scene.ixx:365-377 */
    float Transform[12];
    uint32_t InstanceID;                  /* = InstanceData.FirstGeometryIndex; ObjectIndex = InstanceID + GeometryIndex */
    uint32_t InstanceMask;                /* low 8 bits; 0 hides the instance */
    uint64_t AccelerationStructure;       /* blas id */
} PtInstanceDesc;

/* Top level over all mesh-node instances (BuildTopLevelAccelerationStructure,
 * Source/RaytracingHelpers.ixx:28-74). descs is HOST memory, copied before the call returns. Rebuilds if one already exists.
 * Enqueued on the stream like the reference's build on its command list: instance records, the 8-wide tree over the instance
 * boxes and the traversal copy are made by kernels; a rebuild that needs no more room than the last one allocates nothing and
 * waits for nothing. A tree too deep for the traversal stack is reported by the next pt_sync / render call. */
int  pt_build_top_level(PtContext* ctx, const PtInstanceDesc* descs, uint32_t count, uint32_t build_flags);
/* pt_build_top_level with one addition: for every i with from_device[i] != 0 the instance's transform is read ON THE DEVICE from
 * device_instances[i].ObjectToWorld (what pt_anim_evaluate wrote there, in stream order), not from descs[i].Transform: one small kernel
 * patches the uploaded instance sources in front of the instance-record kernel. from_device is HOST memory, count bytes; device_instances
 * must be the array bound with pt_set_instance_data and reach every instance from_device names (refused otherwise). With
 * from_device NULL or all zero the call IS pt_build_top_level (same launches); device_instances may then be NULL. */
int  pt_build_top_level_posed(PtContext* ctx, const PtInstanceDesc* descs, uint32_t count, uint32_t build_flags,
                              const PtInstanceData* device_instances, const uint8_t* from_device);

/* ------------------------------------------------------------------------------------------
 * animation playback on the device (Source/Animation.ixx: KeyframeCollection::Interpolate :45-75, Animation::ComputeTransforms :119-162;
 * Scene::Refresh, Source/Scene.ixx:195-231). A rig holds the node forest, the clips and the keys of one animation file; an animated
 * object binds a rig to one render object (the reference copies the collection per render object, Scene.ixx:165-168) and owns the
 * device buffers of its results; pt_anim_evaluate poses any number of objects in ONE launch on the context's stream, with no allocation
 * and no wait in the steady state. DESIGN.md section 1, "Animation", is the arithmetic spec (DirectXMath is not part of the reference
 * tree: parity with it is unpinned). Matrices are row-major 4x4 in the reference's row-vector convention unless stated otherwise. The
 * reference matches nodes by NAME; names are resolved to indices by the host (ingest) with the reference's map semantics.
 * All arrays of the create calls are HOST memory, copied during the call.
 * ------------------------------------------------------------------------------------------ */
#define PT_ANIM_NO_NODE 0xFFFFFFFFu
/* One state of pt_anim_evaluate: which object, which clip of its rig, at what time in seconds. 24 B. (Tagged, not a typedef: C callers
 * write `struct PtAnimState`.) */
struct PtAnimState { uint64_t Object; uint32_t Clip; uint32_t _pad; double Time; };
/* parents[node_count]: index of the parent, < the node's own index (depth-first order), -1 for a root.
 * rest_trs[node_count * 10]: Translation[3], Rotation[4] (x, y, z, w), Scale[3] of the node's rest transform.
 * durations[clip_count]; channels[clip_count * node_count * 3 * 2]: per clip, node and path (0 T, 1 R, 2 S) {FirstKey, KeyCount}
 * into key_times[key_count] / key_values[key_count * 4] (T / S keys use xyz); KeyCount 0: the path keeps the rest value.
 * Refused: a parent >= its node, key times of a channel not strictly ascending or not finite, non-finite key values or rest TRS, a
 * channel that runs beyond key_count, a duration that is negative or not finite. */
int  pt_anim_create_rig(PtContext* ctx, uint32_t node_count, const int32_t* parents, const float* rest_trs,
                        uint32_t clip_count, const double* durations, const uint32_t* channels,
                        const float* key_times, const float* key_values, uint32_t key_count, uint64_t* out_rig);
int  pt_anim_release_rig(PtContext* ctx, uint64_t rig);       /* refused while an object refers to it; synchronises */
/* transform16: RenderObject.Transform(). Bindings (one per mesh node of the render object): binding_nodes[i] = the rig node whose
 * global transform moves instance binding_instances[i], or PT_ANIM_NO_NODE: binding_globals16[16 * i] (MeshNode::GlobalTransform) is
 * used instead (Scene.ixx:213). Skins (one per skinned mesh node): skin_mesh_nodes[s] = the rig node of the mesh node (PT_ANIM_NO_NODE:
 * the skin's matrices are never written), skin_joint_counts[s] joints, whose rig nodes (PT_ANIM_NO_NODE: that joint's matrix is never
 * written) and inverse bind matrices follow one another in joint_nodes / inverse_binds16. Matrices never written stay zero. */
int  pt_anim_create_object(PtContext* ctx, uint64_t rig, const float* transform16,
                           uint32_t binding_count, const uint32_t* binding_nodes, const uint32_t* binding_instances, const float* binding_globals16,
                           uint32_t skin_count, const uint32_t* skin_mesh_nodes, const uint32_t* skin_joint_counts,
                           const uint32_t* joint_nodes, const float* inverse_binds16, uint64_t* out_object);
int  pt_anim_release_object(PtContext* ctx, uint64_t object); /* synchronises */
/* Poses states[0 .. count) (HOST memory, staged through a pinned ring like pt_build_top_level's upload): per object the global
 * transform of every node, the skeletal transforms InverseBind . Global(joint) . Global(meshNode)^-1 of every skin (float3x4, the layout
 * pt_skin_mesh reads), and -- when device_instances is not NULL -- for every binding
 *   ObjectToWorld = To3x4(Global(meshNode) . Scale(1, 1, -1) . transform16),  PreviousObjectToWorld = the ObjectToWorld it replaces
 * (on an object's first evaluation: the new ObjectToWorld). device_instances must be the array bound with pt_set_instance_data (its
 * count bounds the bindings' instance indices). A clip with Duration 0 is posed at time 0; a Time beyond the keys clamps per channel.
 * Refused, with nothing modified: an unknown object, an object named twice in one call, a clip out of range, a Time that is not
 * finite, a binding beyond the bound instance data. */
int  pt_anim_evaluate(PtContext* ctx, const struct PtAnimState* states, uint32_t count, PtInstanceData* device_instances);
/* the device array of skin `skin`'s float3x4 matrices (owned by the object, rewritten by every pt_anim_evaluate): goes straight into
 * pt_skin_mesh */
int  pt_anim_skeletal_transforms(PtContext* ctx, uint64_t object, uint32_t skin, const float** device_ptr, uint32_t* joint_count);
/* test aid: the global transforms of the last evaluation, 16 floats per node; out_count = nodes; min(capacity, nodes) matrices are
 * copied. Synchronises. */
int  pt_anim_download_globals(PtContext* ctx, uint64_t object, float* host_dst16, uint32_t capacity, uint32_t* out_count);
/* test aid: skin `skin`'s float3x4 matrices as the last evaluation left them, 12 floats per joint; out_count = joints. Synchronises. */
int  pt_anim_download_skeletal(PtContext* ctx, uint64_t object, uint32_t skin, float* host_dst12, uint32_t capacity, uint32_t* out_count);
/* test aid: the device's slerp on n host cases (q0[4n], q1[4n], t[n]); out[12n]: the result (4), then the intermediates c = dot (after
 * the sign flip), x = 1 - c c, s = sqrtf(x), w = atan2f(s, c), a0 = (1 - t) w, a1 = t w, sinf(a0), sinf(a1) (the last six are 0 on the
 * lerp branch). tests/ measure the error of the device's sqrtf / atan2f / sinf on them. Synchronises. */
int  pt_anim_debug_slerp(PtContext* ctx, const float* q0, const float* q1, const float* t, uint32_t n, float* out);

typedef struct PtAccelStats {
    uint32_t InstanceCount, BottomLevelCount;
    uint64_t TriangleCount;               /* sum over instances */
    uint64_t NodeBytes, TriangleBytes;    /* device memory held by BVH nodes / triangle packets */
    uint32_t NodeSizeBytes, TriangleSizeBytes;   /* 80 (compressed 8-wide node) / 48 */
    uint32_t MaxBottomLevelDepth, TopLevelDepth; /* levels of 8-wide nodes */
    uint64_t BlobBytes;                   /* the traversal copy: instances + every referenced bottom level + top level (0 for a view) */
    uint32_t SharedScene;                 /* 1: this context views another context's scene (pt_share_scene) */
    uint32_t NormalRecords;               /* 1: hits take their vertex normals from the frame's normal records (every instance of a bottom level names the same
                                             vertex data; decided when the object data is resolved), 0: fetched through the hit's own object */
    uint64_t OwnedBottomLevelBytes;       /* nodes + packets + indices of bottom levels held OUTSIDE the traversal copy: updatable ones, and static ones no top level has
                                             seen yet. A static bottom level lives in the copy only (BlobBytes) once a top-level build has adopted it */
    uint32_t RoundObjectsInLds, RoundRecordsInLds;   /* what the fused round kernel stages in LDS behind the traversal copy: objects (resolved geometry + material) |
                                                        normal records; 0 = none: a hit's shading then fetches them from memory (measurement: which bytes reach HBM) */
} PtAccelStats;
int  pt_get_accel_stats(PtContext* ctx, PtAccelStats* out);           /* synchronises */

/* Frames in flight: several contexts (one HIP stream, one set of path queues each) rendering the SAME static scene need one copy
 * of it. After this call `ctx` renders from `source`'s acceleration structures, descriptor table and object / instance data, read-only
 * (reference: one Scene, App.cpp:372-374, whatever the number of frames the swap chain keeps in flight). `ctx` owns none of it:
 * `source` must outlive the sharing, and refuses to rebuild or release its structures while it is viewed. Synchronises both streams. */
int  pt_share_scene(PtContext* ctx, PtContext* source);

/* ------------------------------------------------------------------------------------------
 * per-frame inputs (reference: the GPUBuffers slots the caller fills before each Render,
 * Source/GBufferGeneration.ixx:51, Source/Raytracing.ixx:44; filled at Source/App.cpp:540-561,1016-1074)
 * ------------------------------------------------------------------------------------------ */
int  pt_set_camera(PtContext* ctx, const PtCamera* camera);                          /* host struct, copied */
int  pt_set_scene_data(PtContext* ctx, const PtSceneData* scene_data);               /* host struct, copied */
/* device array, referenced. Material and TextureMapInfoArray are read at every hit; VertexDesc and MeshDescriptors are resolved (and
 * checked against the descriptor heap) when the binding -- pointer or count --, the heap or the instances of the top level change, and
 * after pt_invalidate_object_data. Binding the same pointer and count again (a host that fills its GPUBuffers slots before every Render,
 * Source/App.cpp:540-561) is free and resolves nothing: a caller that REWRITES VertexDesc / MeshDescriptors of a bound array in place says
 * so with pt_invalidate_object_data, and the next render resolves and checks them again (one small kernel + one wait).
 * MeshDescriptors.Indices is checked but not dereferenced at a hit: a triangle's vertex indices are those of the index buffer given to
 * pt_build_bottom_level (kept next to its triangle packets), as DXR itself intersects the triangles of the build-time index buffer. */
int  pt_set_object_data(PtContext* ctx, const PtObjectData* device_objects, uint32_t count);
int  pt_invalidate_object_data(PtContext* ctx);
int  pt_set_instance_data(PtContext* ctx, const PtInstanceData* device_instances, uint32_t count); /* device array, referenced */

/* Multi-GPU framebuffer sharding (not a reference feature). The frame is cut into
 * horizontal bands of BandHeight rows; band b belongs to rank b % RankCount. A context renders
 * only its own bands; its textures hold those rows contiguously (local row = (b / RankCount) *
 * BandHeight + row-in-band). RNG seeds and camera rays use GLOBAL pixel coordinates, so the
 * gathered image is bit-identical to a single-GPU one. RankCount = 1 disables sharding. */
typedef struct PtSharding { uint32_t RankIndex, RankCount, BandHeight, _pad; } PtSharding;
int  pt_set_sharding(PtContext* ctx, const PtSharding* sharding);
int  pt_local_rows(const PtSharding* sharding, uint32_t frame_height, uint32_t* out_rows);
/* The gather (north_star: "image tiles shard naturally across the 8 GPUs of one node with a final RCCL gather over xGMI"; the
 * reference is single-GPU: Source/App.cpp:1157-1329 renders and presents on one device). One communicator per context, i.e. per
 * stream: frames in flight on separate streams never share one. RCCL (librccl.so.1) is loaded at the first of these calls.
 *   pt_comm_get_unique_id  ncclGetUniqueId: PT_COMM_ID_BYTES of host memory, made by one rank and handed to the others by the caller
 *                          (MPI, a file, torch.distributed's store ...)
 *   pt_comm_init           ncclCommInitRank on the context's device; returns when all `world` ranks have called it
 *   pt_comm_adopt          use an ncclComm_t the caller already owns (not destroyed by the library)
 *   pt_comm_destroy        also called by pt_destroy
 *   pt_gather_bands        enqueued on the stream: every non-root rank sends its bands (local_bands: its rows, contiguous, as
 *                          pt_set_sharding lays a texture out), the root receives each band straight into its rows of
 *                          dst_full[H][W] (grouped ncclSend / ncclRecv, one per band, no staging copy) and places its own bands
 *                          with one strided device copy. width * pixel_bytes must be a multiple of 16. Needs a communicator
 *                          whose rank / size equal the sharding's; with RankCount 1 no communicator is needed and nothing is sent.
 * Errors of RCCL come back as PT_ERROR_RCCL with ncclGetErrorString in pt_last_error.
 * pt_gather_plan is the host arithmetic behind it (no GPU, no RCCL): the messages rank sharding->RankIndex issues, in order. With
 * out == NULL only the count is returned. Tests check that the plans of all ranks pair up and tile the frame. */
typedef struct PtBandMessage {
    uint32_t Peer, IsSend, Band, _pad;    /* the other rank | 1 = ncclSend (non-root), 0 = ncclRecv (root) | global band index */
    uint64_t LocalOffset;                 /* byte offset in the sender's local texture */
    uint64_t FullOffset;                  /* byte offset in the root's full frame */
    uint64_t Bytes;
} PtBandMessage;
#define PT_COMM_ID_BYTES 128
int  pt_comm_get_unique_id(void* out_id_host);
int  pt_comm_init(PtContext* ctx, const void* id_host, uint32_t rank, uint32_t world);
int  pt_comm_adopt(PtContext* ctx, void* nccl_comm);
int  pt_comm_destroy(PtContext* ctx);
int  pt_gather_bands(PtContext* ctx, const void* local_bands, void* dst_full, uint32_t width, uint32_t height, uint32_t pixel_bytes, uint32_t root);
int  pt_gather_plan(const PtSharding* sharding, uint32_t height, uint64_t row_bytes, uint32_t root, PtBandMessage* out, uint32_t capacity, uint32_t* out_count);

/* dst_full[H][W] (pixel_bytes each) <- gathered[rank][local rows][W] (what a gather of every rank's
 * local buffer yields, rank r at byte offset rank_offsets[r]). Device pointers; enqueued on the stream. */
int  pt_deinterleave_bands(PtContext* ctx, void* dst_full, const void* gathered, const uint64_t* rank_offsets_host,
                           uint32_t rank_count, uint32_t band_height, uint32_t width, uint32_t height, uint32_t pixel_bytes);

/* ------------------------------------------------------------------------------------------
 * the two operators
 * ------------------------------------------------------------------------------------------ */
/* GBufferGeneration::Render(commandList, topLevelAccelerationStructure, constants),
 * Source/GBufferGeneration.ixx:80-117. Primary pinhole ray per pixel, closest hit, G-buffer stores. */
int  pt_gbuffer_render(PtContext* ctx, const PtGBufferConstants* constants, const PtTextures* textures);

/* Raytracing::SetConstants + Raytracing::Render (Source/Raytracing.ixx:92-112): spp x (Bounces+1)
 * path-tracing loop per pixel, wavefront-scheduled; reads the G-buffer textures written by
 * pt_gbuffer_render for bounce 0 and stores the per-pixel radiance.
 * Vertex normals are read from the objects' vertex buffers once per call, at its start (in stream order), not at every hit:
 * what a hit interpolates is what the buffers held when the call's work began. Tangents, texture coordinates and per-vertex
 * motion are read at the hit. */
int  pt_raytrace_set_constants(PtContext* ctx, const PtGraphicsSettings* settings);
int  pt_raytrace_render(PtContext* ctx, const PtTextures* textures);

/* ------------------------------------------------------------------------------------------
 * direct lighting over emissive triangles (RTXDI::SetConstants + RTXDI::Render, Source/RTXDI.ixx; LightPreparation,
 * DIInitialSampling, DIFinalShading) without temporal / spatial reuse: per pixel LocalLightSamples power-proportional
 * candidates, streaming RIS, one coloured visibility ray. Writes Textures.Diffuse / Specular (R16G16B16A16_FLOAT:
 * radiance.rgb, light distance), which pt_raytrace_render consumes when GraphicsSettings.IsDIEnabled is set; with
 * IsLastRenderPass and Denoiser None / DLSS-RR the result is added to Textures.Radiance instead (DIFinalShading.hlsl:78-103).
 * Reads the G-buffer (LinearDepth, GeometricNormal, NormalRoughness, BaseColorMetalness, IOR, Transmission) and the camera /
 * object data bound for the G-buffer pass. Enqueued on the context's stream; the light list is rebuilt (one wait) only when
 * the instances of the top level, the object-data binding or pt_invalidate_object_data change it.
 * ------------------------------------------------------------------------------------------ */
typedef struct PtDISettings {
    uint32_t RenderSize[2];
    uint32_t FrameIndex;
    uint32_t LocalLightSamples;           /* candidates per pixel, 1..32 (reference default 8) */
    uint32_t Denoiser;                    /* PtDenoiser */
    uint32_t IsLastRenderPass;            /* 1: no path-tracing pass follows (Bounces 0) */
    uint32_t ExtFlags;                    /* PT_EXT_LAMBERTIAN_ONLY honoured */
    uint32_t _pad;
} PtDISettings;                           /* 32 B */

/* One emissive triangle, world space, recomputed at every pt_di_render (TriangleLight::Initialize, Light.hlsli). 80 B. */
typedef struct PtTriangleLight {
    float Base[3], Area;                  /* Area = |Edge0 x Edge1| / 2 (0 for a degenerate triangle) */
    float Edge0[3], Power;                /* Power = Area * pi * luminance(Radiance) (CalculatePower) */
    float Edge1[3]; uint32_t InstanceIndex;
    float Normal[3];                      /* unit (Edge0 x Edge1), 0 when degenerate */
    uint32_t PrimitiveIndex;
    float Radiance[3];                    /* EmissiveColor * EmissiveStrength, times the emissive texture at the UV centroid */
    uint32_t GeometryIndex;
} PtTriangleLight;                         /* 80 B */

int  pt_di_set_constants(PtContext* ctx, const PtDISettings* settings);
int  pt_di_render(PtContext* ctx, const PtTextures* textures);
/* emissive triangles of the current light list (rebuilt first if it is stale); synchronises */
int  pt_di_light_count(PtContext* ctx, uint32_t* out_count);
/* the records of the last pt_di_render, list order (instance, geometry, triangle); synchronises */
int  pt_di_download_lights(PtContext* ctx, PtTriangleLight* host_dst, uint32_t capacity, uint32_t* out_count);

/* ------------------------------------------------------------------------------------------
 * spatiotemporal reservoir reuse of the DI pass (RTXDI's DITemporalResampling / DISpatialResampling, Source/RTXDI.ixx:237-240;
 * defaults of Source/MyAppData.h:226-247). DESIGN.md section 1 is the arithmetic spec; parity with the RTXDI SDK is unpinned.
 * Off by default: pt_di_render is pt_di_render_with_history(ctx, tx, NULL) and, with both passes off, runs the plain pass.
 * Unsharded contexts only. Each context keeps two reservoir buffers of RenderSize pixels x 32 B (ping-ponged per render).
 * ------------------------------------------------------------------------------------------ */
enum { PT_DI_BIAS_CORRECTION_OFF = 0, PT_DI_BIAS_CORRECTION_BASIC = 1 };   /* 2 Pairwise, 3 Raytraced: rejected here; Pairwise is
                                                                             BASIC + pt_di_set_pairwise's *Pairwise flags, Raytraced
                                                                             BASIC + pt_di_set_visibility's *Raytraced flags */
typedef struct PtDIResamplingSettings {
    uint32_t TemporalResampling;          /* 0 / 1 */
    uint32_t TemporalBiasCorrection;      /* OFF | BASIC (reference default BASIC) */
    uint32_t MaxHistoryLength;            /* 1..64, default 20 */
    uint32_t BoilingFilter;               /* 0 / 1, default 1 */
    float    BoilingFilterStrength;       /* [0, 1], default 0.2 */
    float    TemporalDepthThreshold;      /* default 0.1 */
    float    TemporalNormalThreshold;     /* default 0.5 */
    uint32_t SpatialSamples;              /* 0 = no spatial pass, 1..32 (reference default 1) */
    uint32_t SpatialBiasCorrection;       /* OFF | BASIC */
    uint32_t DisocclusionBoostSamples;    /* 0..32, default 8 */
    float    SpatialSamplingRadius;       /* pixels, (0, 64], default 32 */
    float    SpatialDepthThreshold;       /* default 0.1 */
    float    SpatialNormalThreshold;      /* default 0.5 */
    uint32_t _pad[3];
} PtDIResamplingSettings;                 /* 64 B */

typedef struct PtDIReservoir {            /* one per local pixel, row-major */
    uint32_t LightIndex;                  /* into the light list; 0xFFFFFFFF = empty */
    float    U, V;                        /* the two uniforms of Math::SampleTriangle (r1, r2 of the DI spec), unquantised */
    float    W;                           /* unbiased contribution weight */
    uint32_t M;                           /* confidence */
    float    TargetPdf;                   /* p-hat of the sample at this pixel's surface */
    uint32_t Age;                         /* frames since drawn, saturating; informational */
    uint32_t Visibility;                  /* 0 unless pt_di_set_visibility turned a flag on. bits 0-14: rgb visibility, 5 bits per channel,
                                             uint(clamp(v, 0, 1) * 31), decoded / 31; 15-20: dx, 21-26: dy (6-bit two's complement, clamped
                                             to +-31): pixels from where the visibility was traced to this pixel's sample; 27-30: frames
                                             since it was traced, saturating at 15; 31: 0 */
} PtDIReservoir;                          /* 32 B */

typedef struct PtDIPreviousTextures {     /* RTXDI::Textures Previous* members, Source/RTXDI.ixx:37-50: last frame's G-buffer, same formats */
    void* PreviousGeometricNormal; void* PreviousLinearDepth; void* PreviousBaseColorMetalness;
    void* PreviousNormalRoughness; void* PreviousIOR; void* PreviousTransmission;
} PtDIPreviousTextures;

/* NULL or both passes off: the plain pass. A changed value resets the history. */
int  pt_di_set_resampling(PtContext* ctx, const PtDIResamplingSettings* settings);
/* temporal reuse reads previous (not NULL) and Textures.MotionVector; the history is reset on the first render, a RenderSize change,
 * a rebuilt light list and a settings change */
int  pt_di_render_with_history(PtContext* ctx, const PtTextures* textures, const PtDIPreviousTextures* previous);
int  pt_di_reset_history(PtContext* ctx);                                   /* App::ResetHistory */
/* the final reservoirs of the last render (next frame's history), RenderSize pixels row-major; synchronises */
int  pt_di_download_reservoirs(PtContext* ctx, PtDIReservoir* host_dst, uint32_t capacity, uint32_t* out_count);

/* ------------------------------------------------------------------------------------------
 * visibility in the reservoirs (DIInitialSampling.hlsl:49-54, DIFinalShading.hlsl:32-56, RAB_GetConservativeVisibility /
 * RAB_GetTemporalConservativeVisibility, RTXDIAppBridge.hlsli:433-459). DESIGN.md section 1, "Reservoir visibility", is the spec; the
 * defaults are the RTXDI SDK's from memory, unpinned. Takes effect only with reservoir reuse on (the plain pass keeps no reservoir).
 * Every ray is the final-shading ray: surface to sample point, tmin 1e-3, tmax = max(0, distance - 2e-3).
 * ------------------------------------------------------------------------------------------ */
typedef struct PtDIVisibilitySettings {
    uint32_t InitialVisibility;           /* 0 / 1 (SDK default 1): an occluded initial sample empties the reservoir */
    uint32_t FinalVisibilityReuse;        /* 0 / 1 (SDK default 1): final shading reuses a stored visibility instead of tracing */
    uint32_t FinalVisibilityMaxAge;       /* 1..14 frames, default 4 */
    float    FinalVisibilityMaxDistance;  /* pixels, (0, 31], default 16 */
    uint32_t DiscardInvisibleSamples;     /* 0 / 1 (SDK default 0): a sample whose traced final visibility is zero leaves the reservoir */
    uint32_t TemporalRaytraced;           /* 0 / 1: the temporal pass's BASIC normalisation becomes Raytraced */
    uint32_t SpatialRaytraced;            /* 0 / 1: the spatial pass's BASIC normalisation becomes Raytraced */
    uint32_t _pad;
} PtDIVisibilitySettings;                 /* 32 B */
/* NULL or all flags 0: reservoirs carry no visibility (PtDIReservoir.Visibility stays 0). Out-of-range values are refused and leave the
 * previous setting active; a changed value resets the history. A *Raytraced flag whose pass is on with a bias correction other than
 * BASIC is refused by pt_di_render_with_history. */
int  pt_di_set_visibility(PtContext* ctx, const PtDIVisibilitySettings* settings);

/* ------------------------------------------------------------------------------------------
 * pairwise-MIS bias correction of the reuse passes (ReSTIRDI_*BiasCorrectionMode::Pairwise, Source/MyAppData.h:44-59). DESIGN.md
 * section 1, "Pairwise bias correction", is the spec (this library's own; parity with the RTXDI SDK is unpinned). A flag turns the BASIC
 * normalisation of its pass into the pairwise one: one pass over the neighbours, no rays, the pixel's own sample keeps a guaranteed
 * share. It works with pt_di_set_visibility's Visibility word; like BASIC it is biased in penumbrae under initial visibility.
 * ------------------------------------------------------------------------------------------ */
typedef struct PtDIPairwiseSettings {
    uint32_t TemporalPairwise;            /* 0 / 1: the temporal pass's BASIC normalisation becomes Pairwise */
    uint32_t SpatialPairwise;             /* 0 / 1: the spatial pass's BASIC normalisation becomes Pairwise */
    uint32_t Reserved[2];                 /* 0 */
} PtDIPairwiseSettings;                   /* 16 B */
/* NULL or all 0: off. A flag above 1 or a non-zero Reserved is refused and leaves the previous setting active; a changed value resets
 * the history. A flag on a pass that is off is ignored. pt_di_render_with_history refuses a *Pairwise flag whose pass is on with a bias
 * correction other than BASIC, and *Pairwise together with *Raytraced on one pass. */
int  pt_di_set_pairwise(PtContext* ctx, const PtDIPairwiseSettings* settings);

/* ------------------------------------------------------------------------------------------
 * how the initial candidates of the DI pass are drawn (ReSTIRDI.InitialSampling.LocalLight.Mode, Source/MyAppData.h:35-39, 212;
 * ReGIR.Cell.Size / BuildSamples). DESIGN.md section 1, "Local-light sampling", is the arithmetic spec; the RTXDI SDK's static
 * parameters (128 tiles x 1024 lights, 16-pixel screen tiles, a 16 x 16 x 16 grid of 512 lights per cell, jitter 1) are unpinned.
 * POWER_CDF is this library's default and keeps the plain and reuse passes exactly as without this call. POWER_RIS presamples
 * 1 MB of light tiles per render; REGIR_RIS also builds 16 MB of grid cells around the camera Position of the render (points
 * outside the grid fall back to POWER_RIS), or 9.2 MB of Onion cells under pt_di_set_regir_layout. Each context owns its own
 * presampling buffers.
 * ------------------------------------------------------------------------------------------ */
enum { PT_DI_LOCAL_LIGHT_POWER_CDF = 0,   /* this library's default: draw from the power prefix sum */
       PT_DI_LOCAL_LIGHT_UNIFORM   = 1,   /* ReSTIRDI_LocalLightSamplingMode::Uniform */
       PT_DI_LOCAL_LIGHT_POWER_RIS = 2,   /* ::Power_RIS (presampled light tiles) */
       PT_DI_LOCAL_LIGHT_REGIR_RIS = 3 }; /* ::ReGIR_RIS (world-space grid, Power_RIS fallback) */
typedef struct PtDILightSamplingSettings {
    uint32_t Mode;                        /* PT_DI_LOCAL_LIGHT_* (reference default REGIR_RIS) */
    float    ReGIRCellSize;               /* ReGIR.Cell.Size, [0.1, 10], default 1 */
    uint32_t ReGIRBuildSamples;           /* ReGIR.BuildSamples, 1..32, default 8 */
    uint32_t _pad;
} PtDILightSamplingSettings;              /* 16 B */
typedef struct PtDIPresampledLight {
    uint32_t LightIndex;                  /* into the light list; 0xFFFFFFFF = empty */
    float    InvSourcePdf;                /* tiles: total / Power; cells: the ReGIR build's contribution weight */
} PtDIPresampledLight;                    /* 8 B */

/* NULL: POWER_CDF. Out-of-range values are refused and leave the previous setting active; a changed value resets the history. */
int  pt_di_set_light_sampling(PtContext* ctx, const PtDILightSamplingSettings* settings);
/* which = 0: the Power_RIS tiles (tile-major, 128 x 1024), 1: the ReGIR cells (cell-major; Grid: x fastest, 4096 x 512; Onion:
 * 2253 x 512 in the layout's cell order) of the last pt_di_render; out_count = 0 when that render did not fill them; synchronises */
int  pt_di_download_presampled(PtContext* ctx, uint32_t which, PtDIPresampledLight* host_dst, uint32_t capacity, uint32_t* out_count);

/* ------------------------------------------------------------------------------------------
 * the layout of the ReGIR cells (the reference compiles RTXDI_REGIR_MODE RTXDI_REGIR_ONION, Shaders/RTXDIAppBridge.hlsli:6, and
 * fills onionParams in Source/RTXDI.ixx:83-113). GRID, the default: 16 x 16 x 16 cubes of ReGIRCellSize. ONION: 2253 cells around
 * the camera Position -- the sphere of radius c = 0.5 * ReGIRCellSize, then 15 concentric shells out to 145.055 c, each cut into
 * latitude rings and longitude cells (5 layer groups of 8, 12, 16, 20, 24 partitions with 1, 1, 1, 1, 11 layers). The RTXDI SDK is
 * not in the reference tree: the layout is this library's own, after the SDK's structure, unpinned. DESIGN.md section 1,
 * "Local-light sampling", is the spec. The setting acts only in PT_DI_LOCAL_LIGHT_REGIR_RIS; ONION builds 9.2 MB of cells.
 * ------------------------------------------------------------------------------------------ */
enum { PT_DI_REGIR_LAYOUT_GRID = 0, PT_DI_REGIR_LAYOUT_ONION = 1 };
typedef struct PtDIReGIRLayoutSettings {
    uint32_t Layout;                      /* PT_DI_REGIR_LAYOUT_* (reference: ONION) */
    uint32_t _pad[3];
} PtDIReGIRLayoutSettings;                /* 16 B */
/* NULL: GRID. An unknown Layout is refused and leaves the previous setting active; a changed value resets the history. */
int  pt_di_set_regir_layout(PtContext* ctx, const PtDIReGIRLayoutSettings* settings);
/* The Onion layout's static tables at unit scale (host only: no context, no GPU). which = 0: the 16 squared layer boundaries;
 * 1: the ring thresholds sin^2, concatenated by group (20); 2: the azimuth thresholds (pseudo-angles in [0, 4)), concatenated in
 * (group, ring) order (241); 3: the cell spheres, (centre xyz, radius) x 2253. out_count = the number of floats; min(capacity,
 * out_count) floats are copied. */
int  pt_di_regir_onion_table(uint32_t which, float* host_dst, uint32_t capacity, uint32_t* out_count);

/* ------------------------------------------------------------------------------------------
 * BRDF candidates in initial sampling (the reference's BRDFSamples, Source/MyAppData.h:220-221; DESIGN.md section 1, "BRDF
 * candidates", is the spec). On top of the LocalLightSamples light candidates a pixel draws BrdfSamples directions from its all-lobe
 * BSDF (a stream of its own), traces one closest-hit ray each, and a ray that lands on an emissive triangle becomes a light sample of
 * that triangle at the hit point. Light and BRDF candidates are weighted against each other by MIS and stream into one reservoir
 * with M = LocalLightSamples + BrdfSamples; everything behind initial sampling is unchanged. Off by default, and with it off every
 * output is what it was. The RTXDI SDK is not in the reference tree: the arithmetic is this library's own after the structure of
 * RTXDI_SampleBrdf / RTXDI_LightBrdfMisWeight, unpinned.
 * ------------------------------------------------------------------------------------------ */
/* The entry points take plain values and words: the C ABI's list of structs stays the one it was (the ABI tests pin it).
 * brdf_samples: BRDF candidates per pixel, 0..8 (reference default 1); 0: off, whatever brdf_cutoff holds within its range.
 * brdf_cutoff: in [0, 1). > 0: a BRDF ray ends at sqrt((1 / brdf_cutoff - 1) * pdf), and the BRDF pdf of a sample beyond that distance
 * counts as 0 in the MIS weight; 0: rays are unbounded.
 * brdf_samples > 8 and a brdf_cutoff that is negative, not finite or >= 1 are refused and leave the previous setting active; a changed
 * value resets the history. */
int  pt_di_set_brdf_sampling(PtContext* ctx, uint32_t brdf_samples, float brdf_cutoff);
/* The BRDF candidates of the last pt_di_render: local pixels x brdf_samples records, pixel-major, PT_DI_BRDF_CANDIDATE_WORDS 32-bit
 * words each: [0] the light the ray landed on (0xFFFFFFFF: no direction, a miss, or not a light); [1], [2] the float bits of U, V, the
 * hit point as a light sample, U = (b1 + b2)^2, V = b2 / (b1 + b2) (0 without a light); [3] the float bits of the all-lobe pdf of the
 * drawn direction (0 when no direction was drawn). capacity and out_count are in records; out_count = 0 when that render drew none;
 * synchronises. */
#define PT_DI_BRDF_CANDIDATE_WORDS 4u
int  pt_di_download_brdf_candidates(PtContext* ctx, uint32_t* host_dst, uint32_t capacity, uint32_t* out_count);

/* ------------------------------------------------------------------------------------------
 * the local-light PDF texture (App::PrepareReSTIRDI, Source/App.cpp:1095-1116: the LocalLightPDF texture is cleared,
 * LightPreparation writes TriangleLight::CalculatePower() at RTXDI_LinearIndexToZCurve(lightIndex), Shaders/LightPreparation.hlsl:133,
 * and MipmapGeneration::Process builds its chain). With the setting on, every pt_di_render of a scene with emitters builds the texture
 * and its chain, and in PT_DI_LOCAL_LIGHT_POWER_RIS / _REGIR_RIS the Power_RIS tiles come from a descent of the chain
 * (RTXDI_PresampleLocalLights) instead of the power prefix sum, and the source pdf of a light no tile produced
 * (RAB_EvaluateLocalLightSourcePdf, Shaders/RTXDIAppBridge.hlsli:488-501) is Power / (top * M * M), top the chain's last texel and
 * M = max(width, height). POWER_CDF and UNIFORM keep their bits. Off by default, and with it off every launch and output is what it
 * was. The RTXDI SDK is not in the reference tree: size rule and descent are this library's own after the SDK's structure, unpinned;
 * DESIGN.md section 1, "Local-light PDF texture", is the spec (tests/pdfmipref.py restates it). The entry points take plain values and
 * pointers: the C ABI's list of structs stays the one it was.
 * ------------------------------------------------------------------------------------------ */
/* ComputePdfTextureSize (Source/RTXDIResources.ixx:43-52) in integers: width = the smallest power of two >= ceil(sqrt(n)), height = the
 * smallest power of two >= ceil(n / width), mip_levels = log2(max(width, height)) + 1; n = 0 counts as 1; square or 2:1. Host
 * arithmetic, no context, no GPU. light_count above 2^24 and a NULL pointer are refused. */
int  pt_di_pdf_texture_size(uint32_t light_count, uint32_t* width, uint32_t* height, uint32_t* mip_levels);
/* enabled: 0 (the default) or 1; anything else is refused and leaves the previous setting active; a changed value resets the history.
 * The texture is per context (a context viewing a shared scene builds its own), grow-only, 5.6 MB at 2^20 lights. */
int  pt_di_set_pdf_mipmap(PtContext* ctx, uint32_t enabled);
/* One level of the PDF texture of the last pt_di_render, row-major: level k is max(1, width >> k) x max(1, height >> k); level 0
 * holds Power at (x, y) = (even bits, odd bits) of the light index and 0 elsewhere. out_width x out_height = 0 x 0 when that render
 * built none (the setting off, no emitters) or the texture has no such level; min(capacity, out_width * out_height) floats are
 * copied; synchronises. level >= 16 and a NULL out pointer (or a NULL host_dst with capacity > 0) are refused. */
int  pt_di_download_pdf_texture(PtContext* ctx, uint32_t level, float* host_dst, uint32_t capacity, uint32_t* out_width, uint32_t* out_height);

/* ------------------------------------------------------------------------------------------
 * building blocks the reference's direct-lighting bridge calls on the same data
 * ------------------------------------------------------------------------------------------ */
typedef struct PtRayDesc { float Origin[3]; float TMin; float Direction[3]; float TMax; } PtRayDesc;   /* HLSL RayDesc, 32 B */
/* Shadow rays: TraceRay<RAY_FLAG_FORCE_NON_OPAQUE | RAY_FLAG_ACCEPT_FIRST_HIT_AND_END_SEARCH>(q, ray, RAY_FLAG_NONE, ~0u)
 * with the coloured-visibility IsOpaque (Shaders/RaytracingHelpers.hlsli:7-55, Shaders/ShadingHelpers.hlsli:117-159), as used by
 * GetFinalVisibility / GetConservativeVisibility (Shaders/RTXDIAppBridge.hlsli:426-439).
 * device_visibility: 4 floats per ray = visibility.rgb, then 1 if nothing was committed (unoccluded) else 0. */
int  pt_trace_visibility(PtContext* ctx, const PtRayDesc* device_rays, uint32_t count, float* device_visibility);

/* BSDFSample::Evaluate(surfaceVectors, L, V, lobeWeights, diffuse, specular) + EvaluatePDF(...), the all-lobe overloads
 * (Shaders/BxDF.hlsli:247-285) after Initialize + ComputeLobeWeights, batched. */
typedef struct PtBsdfQuery {
    float BaseColor[3], Metallic, Roughness, IOR, Transmission, IsFrontFace;     /* IsFrontFace: 0 or 1 */
    float GeometricNormal[3], ShadingNormal[3], V[3], L[3];
} PtBsdfQuery;                            /* 80 B */
typedef struct PtBsdfResult { float Diffuse[3], Specular[3], PDF, _pad; } PtBsdfResult;   /* 32 B */
int  pt_bsdf_evaluate(PtContext* ctx, const PtBsdfQuery* device_queries, uint32_t count, PtBsdfResult* device_results);
/* One bounce's BSDF step (Shaders/Raytracing.hlsl:326-342): Initialize + ComputeLobeWeights + Sample(random) + the single-lobe
 * EvaluatePDF / Evaluate of the sampled lobe, batched. The material part of the query is laid out as in PtBsdfQuery.
 * Result: the sampled L, the lobe and Sample's return value (Ok); PDF and F are 0 when Ok is 0. */
typedef struct PtBsdfSampleQuery {
    float BaseColor[3], Metallic, Roughness, IOR, Transmission, IsFrontFace;     /* IsFrontFace: 0 or 1 */
    float GeometricNormal[3], ShadingNormal[3], V[3], Random[4];
    uint32_t ExtFlags, _pad[2];                                                  /* PT_EXT_* */
} PtBsdfSampleQuery;                      /* 96 B */
typedef struct PtBsdfSampleResult { float L[3], PDF, F[3], Weights[3]; uint32_t Lobe, Ok; } PtBsdfSampleResult;   /* 48 B */
int  pt_bsdf_sample(PtContext* ctx, const PtBsdfSampleQuery* device_queries, uint32_t count, PtBsdfSampleResult* device_results);

/* ------------------------------------------------------------------------------------------
 * the post-processing chain after the frame (App::PostProcessGraphics with Denoiser::None, Source/App.cpp:1506-1571):
 * Bloom (Source/Bloom.ixx, Shaders/Bloom.hlsl) + Merge (Shaders/Merge.hlsl), DirectXTK's ToneMapPostProcess (App.cpp:1777-1803)
 * and CopyTexture into the R10G10B10A2_UNORM back buffer (App.cpp:1805-1812). DESIGN.md section 1, "Post-processing", is the
 * arithmetic spec; DirectXTK's formulas and Color::ToSrgb are the build's own, unpinned.
 * ------------------------------------------------------------------------------------------ */
enum { PT_TONE_MAP_SATURATE = 1, PT_TONE_MAP_REINHARD = 2, PT_TONE_MAP_ACES_FILMIC = 3 };        /* ToneMapPostProcess::Operator */
enum { PT_COLOR_ROTATION_HDTV_TO_UHDTV = 0, PT_COLOR_ROTATION_DCI_P3_D65_TO_UHDTV = 1,
       PT_COLOR_ROTATION_HDTV_TO_DCI_P3_D65 = 2 };                                                 /* ::ColorPrimaryRotation */
typedef struct PtPostProcessSettings {      /* MyAppData::Settings::Graphics::PostProcessing::{Bloom, ToneMapping} */
    uint32_t RenderSize[2];                 /* 1..16384 each */
    uint32_t IsBloomEnabled;  float BloomStrength;          /* default 1, 0.05; [0, 1] */
    uint32_t IsHDREnabled;                                  /* 0: operator + sRGB estimate (library default); 1: HDR10 */
    uint32_t ToneMappingOperator;  float Exposure;          /* default ACES_FILMIC, 0; [-10, 10] */
    float    PaperWhiteNits;  uint32_t ColorPrimaryRotation;/* default 200 [50, 10000], HDTV_TO_UHDTV */
    uint32_t _pad[3];
} PtPostProcessSettings;                    /* 48 B */
typedef struct PtPostTextures {             /* full-frame, row-major, RenderSize pixels; NULL = not written */
    const void* Radiance;                   /* R16G16B16A16_FLOAT in (required) */
    void* Color;                            /* R16G16B16A16_FLOAT: the tone-mapped texture ToneMap writes */
    void* BackBuffer;                       /* R10G10B10A2_UNORM: what CopyTexture presents */
    void* Display8;                         /* build-side extra: R8G8B8A8_UNORM of Color, for image files */
} PtPostTextures;
/* Out-of-range values and unknown enums are refused (PT_ERROR_INVALID_ARGUMENT) and leave the previous settings active. */
int pt_post_set_constants(PtContext* ctx, const PtPostProcessSettings* settings);
/* Enqueued on the context's stream. Needs no acceleration structure and ignores the sharding (bloom is not local: a sharded host
 * runs it on the gathered frame). Refuses a NULL Radiance, no output bound, and with bloom on a RenderSize below W, H >= 2 and
 * max(W, H) >= 32 (five mips of the half-size pyramid). The pyramid is context-owned and grow-only; a failed allocation returns
 * PT_ERROR_OUT_OF_MEMORY and keeps the previous one. */
int pt_post_render(PtContext* ctx, const PtPostTextures* textures);
/* the image stage s (0..8 of the table) wrote in the last pt_post_render with bloom on; *w = *h = 0 if none; synchronises */
int pt_post_download_bloom(PtContext* ctx, uint32_t stage, uint16_t* host_rgba16f, uint64_t capacity_texels,
                           uint32_t* out_width, uint32_t* out_height);

/* ------------------------------------------------------------------------------------------
 * the NRD composition pass (NRDComposition::Process, Source/NRDComposition.ixx -> Shaders/NRDComposition.hlsl:36-88), which
 * App::ProcessNRD (Source/App.cpp:1595-1688) runs twice around the denoiser: IsPack = 1 turns the path tracer's Diffuse / Specular
 * into the denoiser's input encoding (demodulation by the albedos, hit-distance normalisation, front-end packing), IsPack = 0 unpacks
 * the denoised pair, multiplies the albedos back and adds the result to Radiance. NRD itself stays out of scope: a host brings its
 * own denoiser between the two calls, which sit between pt_raytrace_render and pt_post_render, or runs the library's own filter for
 * the ReLAX packing there (pt_denoiser_process, below). NRD.hlsli is not part of the
 * reference tree: DESIGN.md section 1, "NRD composition", is the arithmetic spec (this library's own after the SDK; parity with the
 * SDK is unpinned; tests/nrdref.py restates it).
 * ------------------------------------------------------------------------------------------ */
struct PtNRDCompositionConstants {          /* NRDComposition::Constants, 8 root constants. (The two structs of this pass are tagged, not
                                               typedefs, like PtAnimState: C callers write `struct PtNRDCompositionConstants`.) */
    uint32_t RenderSize[2];                 /* size of the arrays passed: 1..16384 each */
    uint32_t IsPack;                        /* 0 / 1 */
    uint32_t Denoiser;                      /* PtDenoiser */
    float    ReBLURHitDistance[4];          /* nrd::ReblurSettings().hitDistanceParameters; finite */
};                                          /* 32 B */
struct PtNRDCompositionTextures {           /* NRDComposition::Textures, the same member order; row-major, RenderSize pixels */
    const void *LinearDepth, *DiffuseAlbedo, *SpecularAlbedo, *NormalRoughness;   /* as pt_gbuffer_render writes them */
    void *NoisyDiffuse, *NoisySpecular;     /* R16G16B16A16_FLOAT, rewritten in place by the pack */
    const void *DenoisedDiffuse, *DenoisedSpecular;
    void *Radiance;                         /* R16G16B16A16_FLOAT, += by the compose (its alpha keeps its bits) */
};
/* Enqueued on the context's stream. Needs no acceleration structure. One lane moves two pixels with 16-byte accesses when every texture
 * of the call is aligned to two texels (16 bytes; LinearDepth 8), else one pixel with 8-byte accesses: the same bytes either way.
 * The pass is element-wise and ignores the sharding: a sharded context passes its own rows and their size. The pack needs
 * LinearDepth, both albedos and both Noisy*, plus NormalRoughness when Denoiser is ReBLUR; the compose needs LinearDepth, both
 * albedos, both Denoised* and Radiance. Denoised* may point at Noisy* (the identity denoiser, no copy). A pixel whose LinearDepth
 * is not finite is left untouched in every texture. Refused with PT_ERROR_INVALID_ARGUMENT and a message that names the field,
 * nothing written: a missing binding, a texture not aligned to its texel (8 bytes; LinearDepth 4), an unknown Denoiser,
 * IsPack > 1, a RenderSize out of range, a ReBLURHitDistance that is not finite. */
int  pt_nrd_composition_process(PtContext* ctx, const struct PtNRDCompositionConstants* constants, const struct PtNRDCompositionTextures* textures);
/* The pixels per lane of the kernel that call would launch: 2 or 1; 0 when the call would be refused. Host arithmetic on the pointer
 * values (nothing is dereferenced, no GPU): the decision pt_nrd_composition_process itself takes. */
int  pt_nrd_composition_pixels_per_lane(const struct PtNRDCompositionConstants* constants, const struct PtNRDCompositionTextures* textures);
void pt_nrd_reblur_hit_distance_defaults(float out[4]);    /* {3, 0.1, 20, -25}; needs no GPU */

/* ------------------------------------------------------------------------------------------
 * the denoiser for the ReLAX slot between the two calls of the composition pass: this library's own filter in ReLAX's shape (temporal
 * accumulation with reprojection, a variance estimate, an edge-stopping a-trous wavelet), NOT a port of NRD's ReLAX, whose source is
 * not part of the reference tree. DESIGN.md section 1, "Denoiser", is the arithmetic spec (unpinned against the SDK; tests/denoiseref.py
 * restates it bit for bit). It reads the ReLAX-packed pair (radiance, hit distance) and the G-buffer guides and writes a pair in the
 * same encoding. ReBLUR's packing (YCoCg, normalised hit distance) is not served.
 * ------------------------------------------------------------------------------------------ */
struct PtDenoiserSettings {           /* (tagged, not a typedef, like the structs of the composition pass: C callers write `struct PtDenoiserSettings`) */
    uint32_t RenderSize[2];            /* 1..16384 each */
    uint32_t MaxAccumulatedFrames;     /* default 30; 1..255 (1 = no temporal reuse) */
    uint32_t AtrousIterations;         /* default 5; 0..8 (0 = temporal stage only) */
    float    DepthThreshold;           /* default 0.01; (0, 1]: relative, both for reprojection and for the plane distance */
    float    NormalCosine;             /* default 0.8; [0, 1): taps whose normals agree less weigh 0 */
    float    DiffuseLuminanceSigma;    /* default 2;  > 0 */
    float    SpecularLuminanceSigma;   /* default 1;  > 0 */
    float    RoughnessFraction;        /* default 0.15; > 0: specular taps, relative roughness difference that weighs 0 */
    uint32_t _pad[3];
};                                     /* 48 B */
struct PtDenoiserTextures {            /* full frame, row-major, RenderSize pixels */
    const void *Position, *LinearDepth, *NormalRoughness, *MotionVector;   /* as pt_gbuffer_render writes them */
    const void *NoisyDiffuse, *NoisySpecular;                              /* R16G16B16A16_FLOAT, ReLAX-packed (radiance, hit distance) */
    void *DenoisedDiffuse, *DenoisedSpecular;                              /* same format; may alias the Noisy pair */
};
/* Out-of-range values are refused (PT_ERROR_INVALID_ARGUMENT, the message names the field) and leave the previous settings active.
 * Settings that differ from the active ones (RenderSize among them) restart the history. */
int pt_denoiser_set_constants(PtContext* ctx, const struct PtDenoiserSettings* settings);
/* One frame: 2 + AtrousIterations launches enqueued on the context's stream (1 when AtrousIterations is 0). Needs no scene and ignores
 * the sharding (the filter is not local: a sharded host runs it on the gathered frame). A pixel whose LinearDepth is not finite is
 * copied from Noisy* to Denoised* bit for bit. The history (fp32 accumulated colours and hit distances, luminance moments, lengths, the
 * previous frame's guides, the a-trous ping-pong: 272 B per pixel) is context-owned and grow-only; a failed allocation returns
 * PT_ERROR_OUT_OF_MEMORY and keeps what was there. It restarts on the first call, after pt_denoiser_reset_history and after a change
 * of settings. Refused with PT_ERROR_INVALID_ARGUMENT and a message that names the field, nothing written and the history untouched:
 * a NULL binding, a texture not aligned to its texel (Position 16 bytes, LinearDepth 4, the others 8), a call before
 * pt_denoiser_set_constants. */
int pt_denoiser_process(PtContext* ctx, const struct PtDenoiserTextures* textures);
int pt_denoiser_reset_history(PtContext* ctx);
/* Test aid: the accumulated length of the diffuse channel per pixel after the last pt_denoiser_process (0: the G-buffer missed), the
 * first min(capacity_pixels, w * h) of them; *out_w = *out_h = 0 when there is no history. Synchronises. */
int pt_denoiser_download_history(PtContext* ctx, float* host_length, uint64_t capacity_pixels, uint32_t* out_w, uint32_t* out_h);

/* Two more bits of pt_set_debug_flags, for tests and A/B runs: which form of the a-trous kernel pt_denoiser_process launches. */
#define PT_DENOISER_FORM_DIRECT 0x800u   /* every a-trous step takes the direct form (each tap a global load) */
#define PT_DENOISER_FORM_STAGED 0x1000u  /* the staged form (tile + halo through LDS) at every step whose halo fits (1, 2, 4): what the library chooses
                                            unasked, since it is the faster one there. The same bytes either way */

/* ------------------------------------------------------------------------------------------
 * the temporal upscaler for the super-resolution slot of App::PostProcessGraphics (Source/App.cpp:1532-1541), between the denoiser and
 * Bloom / ToneMap: this library's own temporal accumulating upscaler (TAAU) from RenderSize to OutputSize, NOT a port of DLSS or XeSS,
 * which the reference loads there (closed SDKs, not part of its tree). DESIGN.md section 1, "Upscaler", is the arithmetic spec (unpinned
 * against either SDK; tests/upscaleref.py restates it bit for bit). It reads what the reference hands its upscaler: Radiance,
 * MotionVector and LinearDepth at RenderSize and the frame's Camera.Jitter (as it stands in PtCamera: not negated), and writes Color at
 * OutputSize, which then is the post chain's Radiance.
 * ------------------------------------------------------------------------------------------ */
struct PtUpscalerSettings {            /* (tagged, not a typedef, like PtDenoiserSettings: C callers write `struct PtUpscalerSettings`) */
    uint32_t RenderSize[2];            /* 1..16384 each */
    uint32_t OutputSize[2];            /* 1..16384 each; RenderSize <= OutputSize <= 4 RenderSize per axis */
    uint32_t MaxAccumulatedFrames;     /* default 16; 1..255 (1 = no temporal reuse) */
    float    KernelRadius;             /* default 1; [0.75, 2]: the radius of the reconstruction kernel, in render pixels */
    float    DepthThreshold;           /* default 0.01; (0, 1]: relative depth difference beyond which a history tap is rejected */
    uint32_t _pad[5];
};                                     /* 48 B */
struct PtUpscalerTextures {            /* full frames, row-major */
    const void *Radiance, *LinearDepth, *MotionVector;   /* RenderSize: R16G16B16A16_FLOAT (alpha ignored), R32_FLOAT, R16G16B16A16_FLOAT, as the frame wrote them */
    void *Color;                                         /* OutputSize: R16G16B16A16_FLOAT, alpha 1; must not overlap the inputs */
};
enum PtSuperResolutionMode {           /* SuperResolutionMode of Source/Upscaler.ixx, in its order */
    PT_SUPER_RESOLUTION_AUTO = 0, PT_SUPER_RESOLUTION_NATIVE = 1, PT_SUPER_RESOLUTION_QUALITY = 2, PT_SUPER_RESOLUTION_BALANCED = 3,
    PT_SUPER_RESOLUTION_PERFORMANCE = 4, PT_SUPER_RESOLUTION_ULTRA_PERFORMANCE = 5
};
/* Out-of-range values are refused (PT_ERROR_INVALID_ARGUMENT, the message names the field) and leave the previous settings active.
 * Settings that differ from the active ones (a size among them) restart the history. */
int pt_upscaler_set_constants(PtContext* ctx, const struct PtUpscalerSettings* settings);
/* One frame: one launch enqueued on the context's stream. jitter is the Camera.Jitter the frame was rendered with. Needs no scene. The
 * history (fp32 colour in the tone-mapped space, accumulated weight n and depth, two parities: 40 B per output pixel) is context-owned
 * and grow-only; a failed allocation returns PT_ERROR_OUT_OF_MEMORY and keeps what was there. It restarts on the first call, after
 * pt_upscaler_reset_history and after a change of settings. Refused with PT_ERROR_INVALID_ARGUMENT and a message that names the field,
 * nothing written and the history untouched: a NULL binding, a texture not aligned to its texel (LinearDepth 4 bytes, the others 8), a
 * jitter that is not finite or outside [-0.5, 0.5], a call before pt_upscaler_set_constants, a sharded context (the pass is not local:
 * a sharded host runs it on the gathered frame of an unsharded context). */
int pt_upscaler_process(PtContext* ctx, const struct PtUpscalerTextures* textures, const float jitter[2]);
int pt_upscaler_reset_history(PtContext* ctx);
/* Test aid: the accumulated weight n per output pixel after the last pt_upscaler_process, the first min(capacity_pixels, w * h) of
 * them; *out_w = *out_h = 0 when there is no history. Synchronises. */
int pt_upscaler_download_history(PtContext* ctx, float* host_length, uint64_t capacity_pixels, uint32_t* out_w, uint32_t* out_h);
/* Host only, no GPU and no context. The render size of a mode for an output size, max(1, (output * 10 + r10 / 2) / r10) per axis in
 * integers with r10 = 10, 15, 17, 20, 30 for NATIVE .. ULTRA_PERFORMANCE (the ratios the SDKs publish: unpinned); AUTO resolves by
 * the output's pixel count (App.cpp:1427-1440). */
int pt_upscaler_render_size(uint32_t mode, const uint32_t output[2], uint32_t render_out[2]);
/* Host only. The Camera.Jitter of a frame: the Halton point (bases 2 and 3) of index frame_index % count + 1, minus 0.5 per axis, in
 * [-0.5, 0.5); count = ceil(8 (ow / rw) (oh / rh)) in fp32 (App.cpp:661). The radical inverse is this library's own fp32 loop. */
int pt_upscaler_jitter(uint64_t frame_index, const uint32_t render[2], const uint32_t output[2], float jitter_out[2]);

/* Two more bits of pt_set_debug_flags, for tests and A/B runs: which form of the kernel pt_upscaler_process launches. */
#define PT_UPSCALER_FORM_DIRECT 0x2000u  /* the direct form (each tap a global load) */
#define PT_UPSCALER_FORM_STAGED 0x4000u  /* the staged form (the tile's render footprint and halo through LDS): what the library chooses unasked, since it
                                            is the faster one at a 4K output and level at 1080p. The same bytes either way */

/* ------------------------------------------------------------------------------------------
 * the denoising upscaler for the ray-reconstruction slot of App::PostProcessGraphics (Source/App.cpp:1513-1523, :1700-1716), which the
 * reference's default settings (Denoiser = DLSSRayReconstruction) fill with ProcessDLSSRayReconstruction: this library's own filter,
 * NOT a port of DLSS Ray Reconstruction (a closed SDK, not part of the reference tree). DESIGN.md section 1, "Ray reconstruction", is the
 * arithmetic spec (unpinned against the SDK; tests/reconstructref.py restates it bit for bit). It reads what the frame wrote for
 * PT_DENOISER_DLSS_RAY_RECONSTRUCTION at RenderSize -- the noisy Radiance (one signal, direct + indirect), the two albedos,
 * NormalRoughness, Position, LinearDepth, MotionVector -- and the frame's Camera.Jitter (as it stands in PtCamera: not negated), and
 * writes the denoised Color at OutputSize, which then is the post chain's Radiance. The signal is Radiance divided by the albedo sum
 * (floored at 1/64 per channel); it is accumulated over time, filtered by an edge-stopping a-trous wavelet, and multiplied by each
 * tap's own albedo again inside the temporal resolve to OutputSize. SpecularHitDistance is not read: reprojection follows the surface
 * motion only (no virtual motion), as in the denoiser.
 * ------------------------------------------------------------------------------------------ */
struct PtReconstructionSettings {      /* (tagged, not a typedef, like PtDenoiserSettings: C callers write `struct PtReconstructionSettings`) */
    uint32_t RenderSize[2];            /* 1..16384 each */
    uint32_t OutputSize[2];            /* 1..16384 each; RenderSize <= OutputSize <= 4 RenderSize per axis */
    uint32_t MaxAccumulatedFrames;     /* default 30; 1..255: the history of the signal at RenderSize (1 = no temporal reuse there) */
    uint32_t MaxOutputFrames;          /* default 16; 1..255: the history of the output at OutputSize */
    uint32_t AtrousIterations;         /* default 5; 0..8 (0 = no spatial filter) */
    float    DepthThreshold;           /* default 0.01; (0, 1]: relative, for both reprojections and for the plane distance */
    float    NormalCosine;             /* default 0.8; [0, 1): taps whose normals agree less weigh 0 */
    float    LuminanceSigma;           /* default 2;  > 0 */
    float    RoughnessFraction;        /* default 0.15; > 0: relative roughness difference that weighs 0 */
    float    KernelRadius;             /* default 1; [0.75, 2]: the radius of the resolve's reconstruction kernel, in render pixels */
    uint32_t _pad[4];
};                                     /* 64 B */
struct PtReconstructionTextures {      /* full frames, row-major */
    const void *Radiance, *DiffuseAlbedo, *SpecularAlbedo;                 /* RenderSize, R16G16B16A16_FLOAT (alpha ignored), as the frame wrote them */
    const void *NormalRoughness, *Position, *LinearDepth, *MotionVector;   /* RenderSize, as pt_gbuffer_render writes them */
    void *Color;                                                           /* OutputSize: R16G16B16A16_FLOAT, alpha 1; must not overlap an input */
};
/* Out-of-range values are refused (PT_ERROR_INVALID_ARGUMENT, the message names the field) and leave the previous settings active.
 * Settings that differ from the active ones (a size among them) restart the history. */
int pt_reconstruction_set_constants(PtContext* ctx, const struct PtReconstructionSettings* settings);
/* One frame: 3 + AtrousIterations launches enqueued on the context's stream. jitter is the Camera.Jitter the frame was rendered with
 * (pt_upscaler_render_size and pt_upscaler_jitter serve this pass too). Needs no scene. A pixel whose LinearDepth is not finite is
 * never filtered: its Radiance (all three channels 0 when one is not finite) goes to the resolve as it is. The history is context-owned
 * and grow-only, and apart from the upscaler's (a context may run both): per render pixel 160 B (fp32 signal and length, luminance
 * moments and guide records in two parities, the albedo, the a-trous ping-pong), per output pixel 40 B (fp32 colour in the tone-mapped
 * space, accumulated weight n and depth, two parities). A failed allocation returns PT_ERROR_OUT_OF_MEMORY and keeps what was there.
 * It restarts on the first call, after pt_reconstruction_reset_history and after a change of settings. Refused with
 * PT_ERROR_INVALID_ARGUMENT and a message that names the field, nothing written and the history untouched: a NULL binding, a texture
 * not aligned to its texel (Position 16 bytes, LinearDepth 4, the others 8), Color overlapping an input, a jitter that is not finite or
 * outside [-0.5, 0.5], a call before pt_reconstruction_set_constants, a sharded context (the pass is not local: a sharded host runs it
 * on the gathered frame of an unsharded context). */
int pt_reconstruction_process(PtContext* ctx, const struct PtReconstructionTextures* textures, const float jitter[2]);
int pt_reconstruction_reset_history(PtContext* ctx);
/* Test aid, after the last pt_reconstruction_process: host_length, the history length of the signal per render pixel (0: the G-buffer
 * missed); host_filtered, four floats per render pixel, what the resolve read (the filtered signal and its variance; the guarded
 * Radiance and 0 where the G-buffer missed); host_n, the accumulated weight n per output pixel. The first min(capacity, w * h) pixels
 * of each; a NULL array is skipped. render_out = output_out = 0 x 0 when there is no history. Synchronises. */
int pt_reconstruction_download_history(PtContext* ctx, float* host_length, float* host_filtered, uint64_t capacity_render_pixels,
                                       float* host_n, uint64_t capacity_output_pixels, uint32_t render_out[2], uint32_t output_out[2]);

/* Two more bits of pt_set_debug_flags, for tests and A/B runs: which form of the a-trous kernel pt_reconstruction_process launches. */
#define PT_RECONSTRUCTION_FORM_DIRECT 0x8000u   /* every a-trous step takes the direct form (each tap a global load) */
#define PT_RECONSTRUCTION_FORM_STAGED 0x10000u  /* the staged form (tile + halo through LDS) at every step whose halo fits (1, 2, 4): what the library
                                                   chooses unasked. The same bytes either way */

/* ------------------------------------------------------------------------------------------
 * the frame interpolator for the frame-generation slot of App::PostProcessGraphics (Source/App.cpp:1564-1566, :1719-1726), which the
 * reference's default settings (IsDLSSFrameGenerationEnabled = true, MyAppData.h:295) fill with DLSS-G after the tone-mapped copy: this
 * library's own motion-compensated interpolator, NOT a port of DLSS-G or FSR 3 (closed or foreign SDKs, not part of the reference tree)
 * and unpinned against both. DESIGN.md section 1, "Frame generation", is the arithmetic spec (tests/framegenref.py restates it bit for
 * bit). It reads what the reference tags for DLSS-G -- the tone-mapped Color at OutputSize, LinearDepth and MotionVector at RenderSize
 * -- and the frame's Camera.Jitter (as it stands in PtCamera: not negated), keeps the frame before it, and writes the frame at phase
 * Phase between the two. No optical flow, UI mask, reactive mask or presentation pacing: a host displays Generated, then Color.
 * ------------------------------------------------------------------------------------------ */
struct PtFrameGenerationSettings {     /* (tagged, not a typedef, like PtUpscalerSettings: C callers write `struct PtFrameGenerationSettings`) */
    uint32_t RenderSize[2];            /* 1..16384 each: the size of LinearDepth and MotionVector */
    uint32_t OutputSize[2];            /* 1..16384 each; RenderSize <= OutputSize <= 4 RenderSize per axis: the size of Color and Generated */
    float    Phase;                    /* default 0.5; (0, 1): 0 would be the previous frame, 1 the current one */
    float    DepthThreshold;           /* default 0.01; (0, 1]: relative depth difference beyond which a warped sample is rejected */
    uint32_t _pad[6];
};                                     /* 48 B */
struct PtFrameGenerationTextures {     /* full frames, row-major */
    const void *Color;                                   /* OutputSize: R16G16B16A16_FLOAT, what pt_post_render writes as Color (taken as unjittered) */
    const void *LinearDepth, *MotionVector;              /* RenderSize: R32_FLOAT, R16G16B16A16_FLOAT, as pt_gbuffer_render writes them */
    void *Generated;                                     /* OutputSize: R16G16B16A16_FLOAT, alpha 1; must not overlap an input */
    void *Generated8;                                    /* optional (NULL: not written): R8G8B8A8_UNORM of Generated, by the rule of PtPostTextures.Display8 */
};
enum PtFrameGenerationClass {          /* the class byte of an output pixel (pt_frame_generation_download_field) */
    PT_FRAME_GENERATION_BOTH = 0, PT_FRAME_GENERATION_CURRENT_ONLY = 1, PT_FRAME_GENERATION_PREVIOUS_ONLY = 2, PT_FRAME_GENERATION_FALLBACK = 3
};
/* Out-of-range values are refused (PT_ERROR_INVALID_ARGUMENT, the message names the field) and leave the previous settings active.
 * Settings that differ from the active ones (a size among them) drop the previous frame. */
int pt_frame_generation_set_constants(PtContext* ctx, const struct PtFrameGenerationSettings* settings);
/* One frame, enqueued on the context's stream: the clear of the field, the scatter, the resolve, then the copy of Color and LinearDepth
 * into the context (the caller may overwrite its textures once the call returned). jitter is the Camera.Jitter the frame was rendered
 * with. Needs no scene. The first call after creation, after pt_frame_generation_reset_history and after a change of settings has no
 * previous frame: it copies Color to Generated bit for bit (Generated8 from it), keeps the frame and sets *out_generated = 0; later
 * calls set it to 1. Context-owned and grow-only: the previous Color (8 B per output pixel), the previous LinearDepth (4 B per render
 * pixel), the midpoint field (8 B per render pixel), the class bytes of the test aid (1 B per output pixel); the previous jitter is
 * kept beside them. A failed allocation returns PT_ERROR_OUT_OF_MEMORY and changes nothing. Refused with PT_ERROR_INVALID_ARGUMENT and
 * a message that names the field, nothing written and the history untouched: a NULL required binding (out_generated among them), a
 * texture not aligned to its texel (LinearDepth and Generated8 4 bytes, the others 8), Generated or Generated8 overlapping an input or
 * each other, a jitter that is not finite or outside [-0.5, 0.5], a call before pt_frame_generation_set_constants, a sharded context
 * (the pass is not local: a sharded host runs it on the gathered frame of an unsharded context). */
int pt_frame_generation_process(PtContext* ctx, const struct PtFrameGenerationTextures* textures, const float jitter[2], uint32_t* out_generated);
int pt_frame_generation_reset_history(PtContext* ctx);
/* Test aid, after the last pt_frame_generation_process that generated a frame: host_field, the midpoint field, one 64-bit word per
 * render pixel (bits(z) << 32 | index of the render pixel that won the cell; all ones: no surface landed there); host_class, one
 * PtFrameGenerationClass byte per output pixel. The first min(capacity, w * h) of each; a NULL array is skipped. render_out =
 * output_out = 0 x 0 when the last call generated nothing. Synchronises. */
int pt_frame_generation_download_field(PtContext* ctx, uint64_t* host_field, uint64_t capacity_render_pixels, uint8_t* host_class,
                                       uint64_t capacity_output_pixels, uint32_t render_out[2], uint32_t output_out[2]);

/* ------------------------------------------------------------------------------------------
 * the sharpening filter for the image-scaling slot of App::PostProcessGraphics (App::ProcessNIS, Source/App.cpp:1544-1548, :1756-1766),
 * which the reference fills with NVIDIA Image Scaling in its sharpen mode (sl::NISMode::eSharpen, NIS.Sharpness, MyAppData.h:297-303)
 * between the upscaler and Bloom: this library's own edge-adaptive sharpener, NOT a port of NVIDIA Image Scaling (Streamline's NIS
 * plugin, a binary the reference tree does not carry) and unpinned against it. DESIGN.md section 1, "Sharpening", is the arithmetic
 * spec (tests/sharpenref.py restates it bit for bit). It works on the linear HDR colour the post chain would otherwise read: a
 * high-pass along the row, the column and the two diagonals of the 5 x 5, combined by the luminance gradient across each (across the
 * edge, not along it), gated by the Michelson contrast of the 3 x 3 and limited to the 3 x 3 range of the input (no overshoot). No
 * scaler mode, no chromatic aberration, no history, no context-owned memory.
 * ------------------------------------------------------------------------------------------ */
struct PtSharpenSettings {             /* (tagged, not a typedef, like PtUpscalerSettings: C callers write `struct PtSharpenSettings`) */
    uint32_t Size[2];                  /* 1..16384 each: the size of Color and Sharpened, the size the post chain runs at */
    float    Sharpness;                /* default 0.5; [0, 1]: the reference's NIS.Sharpness and its clamp; 0 returns the (guarded) input */
    float    ContrastFloor;            /* default 0.015625; [2^-10, 0.5]: the 3 x 3's Michelson contrast below which nothing is sharpened; full strength at twice it */
    uint32_t _pad[4];
};                                     /* 32 B */
struct PtSharpenTextures {             /* full frames, row-major */
    const void *Color;                 /* R16G16B16A16_FLOAT, linear HDR: what pt_post_render would read as Radiance */
    void *Sharpened;                   /* R16G16B16A16_FLOAT, alpha 1; must not overlap Color */
};
/* Out-of-range or non-finite values are refused (PT_ERROR_INVALID_ARGUMENT, the message names the field) and leave the previous settings
 * active. */
int pt_sharpen_set_constants(PtContext* ctx, const struct PtSharpenSettings* settings);
/* One frame, one kernel enqueued on the context's stream. Needs no scene and allocates nothing. Ignores the sharding, as pt_post_render
 * does: the taps reach two rows beyond a band, so a sharded host runs it on the gathered frame. Refused with PT_ERROR_INVALID_ARGUMENT
 * and a message, nothing written: NULL textures or a NULL texture, a texture not aligned to its texel (8 bytes), Sharpened overlapping
 * Color (the taps read neighbours), a call before pt_sharpen_set_constants. */
int pt_sharpen_process(PtContext* ctx, const struct PtSharpenTextures* textures);

/* ------------------------------------------------------------------------------------------
 * the mip chain of an R32_FLOAT texture (MipmapGeneration::SetTexture + Process, Source/MipmapGeneration.ixx ->
 * Shaders/MipmapGeneration.hlsl), which App::PrepareReSTIRDI (Source/App.cpp:1095-1116) runs on the LocalLightPDF texture. The
 * shader is not restated: DESIGN.md section 1, "Local-light PDF texture", is the arithmetic spec (tests/pdfmipref.py restates it).
 * ------------------------------------------------------------------------------------------ */
/* levels: a host array of mip_levels device pointers; levels[k] is level k, row-major and tightly packed, max(1, width >> k) x
 * max(1, height >> k) texels. Level 0 is read, levels 1 .. mip_levels - 1 are written: a texel is a quarter of the sum of the four
 * under it, a texel outside its level counting as 0 (the levels of a 2:1 texture stay zero-padded to a square). Unlike the reference's
 * Process, which under-dispatches its second pass for textures wider than 1024, every level is covered fully. Enqueued on the
 * context's stream, ceil((mip_levels - 1) / 5) launches; mip_levels = 1 enqueues nothing. Needs no scene. Refused with
 * PT_ERROR_INVALID_ARGUMENT and a message, nothing enqueued: a NULL array or level, a level not aligned to 4 bytes, a width or height
 * that is 0, not a power of two or above 16384, mip_levels of 0, above 16 or above log2(max(width, height)) + 1. */
int  pt_mipmap_generate(PtContext* ctx, float* const* levels, uint32_t width, uint32_t height, uint32_t mip_levels);

/* ------------------------------------------------------------------------------------------
 * the SHARC radiance cache: the Raytracing::Render overload with RTXGITechnique::SHARC (Source/Raytracing.ixx:114-148, Source/SHARC.ixx,
 * the SHARC_UPDATE / SHARC_QUERY permutations of Shaders/Raytracing.hlsl). A world-space hash grid of radiance: an update pass walks one
 * path per DownscaleFactor^2 pixels and deposits what it finds, a resolve pass blends the frame into the history, and the query pass -- the
 * plain estimator -- ends a sample at its first far-and-blurred-enough hit on a voxel that holds samples. The SDK's headers are not part of
 * the reference tree: grid, map, voxel word, resolve and anti-firefly rules are this library's own ("Radiance cache";
 * tests/sharcref.py restates them), unpinned. PtGraphicsSettings.SHARC stays ignored: the cache is switched on by these calls alone.
 * ------------------------------------------------------------------------------------------ */
typedef struct PtSHARCSettings {            /* SHARC::Constants + Raytracing::SHARCSettings */
    uint32_t AccumulationFrames;            /* default 10; 1..63 */
    uint32_t MaxStaleFrames;                /* default 64; 1..255 (a voxel is dropped after max(this, 8) frames without a sample) */
    float    SceneScale;                    /* default 50; [5, 100] */
    uint32_t IsAntiFireflyEnabled;          /* the reference passes 1; 0 or 1 */
    uint32_t DownscaleFactor;               /* 1..4, default 4: the update pass covers (W / f) x (H / f) pixels */
    float    RoughnessThreshold;            /* default 0.4; [0, 1] */
    uint32_t IsHashGridVisualizationEnabled;/* must be 0 */
} PtSHARCSettings;                          /* 28 B */
typedef struct PtSHARCEntry { uint64_t Key; uint32_t Voxel[4]; uint32_t _pad[2]; } PtSHARCEntry;   /* 32 B: a live entry: radiance sums x 1e3 | samples, frames << 18, stale << 24 */
typedef struct PtSHARCQueryResult { uint32_t Valid; float Radiance[3]; } PtSHARCQueryResult;       /* 16 B */
typedef struct PtSHARCPathVertex {          /* one bounce of one update path (pt_sharc_download_update_paths) */
    float Position[3]; uint32_t Flags;      /* PT_SHARC_VERTEX_*; 0: the path never got here */
    float Normal[3];   float Random;        /* the front flat normal | the random number of the hit update */
    float Radiance[3]; uint32_t KeyLo;      /* the radiance term handed to the hit / miss update | the device's key of the vertex */
    float Throughput[3]; uint32_t KeyHi;    /* the bounce's throughput handed to SetThroughput (when not ENDED) */
} PtSHARCPathVertex;                        /* 64 B */
typedef struct PtSHARCPathScatter {         /* the BSDF step of the same bounce (pt_sharc_download_update_scatter) */
    PtBsdfSampleQuery Query;                /* what pt_bsdf_sample needs to repeat it: the material as BSDFSample::Initialize took it, Roughness
                                               after the RoughnessThreshold floor, the frame, V, the four draws, ExtFlags */
    float Origin[3]; uint32_t Sampled;      /* the origin of the ray that follows (GetSafeWorldRayOrigin) | 1: the step ran (0: the path ended before it) */
    float L[3];      uint32_t Goes;         /* the sampled direction | 1: the path went on after the step */
} PtSHARCPathScatter;                       /* 128 B */
#define PT_SHARC_VERTEX_HIT       0x1u
#define PT_SHARC_VERTEX_MISS      0x2u
#define PT_SHARC_VERTEX_ENDED     0x4u      /* the path ended at this vertex: SetThroughput was not reached */
#define PT_SHARC_VERTEX_RESAMPLED 0x8u      /* ... because the hit update took the voxel's history instead of going on */
/* SHARC::Configure: allocates HashEntries (8 B), VoxelData and PreviousVoxelData (16 B each) per entry, context-owned, and empties them.
 * capacity 0 = 1 << 22; it must be a multiple of 32 (the bucket). Synchronises when it replaces a cache. */
int pt_sharc_configure(PtContext* ctx, uint32_t capacity);
/* Out-of-range fields are refused (PT_ERROR_INVALID_ARGUMENT) and leave the previous settings active. */
int pt_sharc_set_constants(PtContext* ctx, const PtSHARCSettings* settings);
/* The Render overload: clear VoxelData, update, resolve, query (the frame, with pt_raytrace_set_constants' GraphicsSettings), swap.
 * PT_ERROR_NOT_READY before pt_sharc_configure / pt_sharc_set_constants. Refuses a sharded context (the cache is world-space and global, a
 * band holds only its own G-buffer rows), the NRD denoisers (None and DLSS-RR are served) and the PT_DEBUG_BRUTE_FORCE / _TRAVERSAL_V1
 * traversals (they keep no hit distance). The cached and the plain frame have launch sequences of their own: a context that alternates
 * pt_raytrace_render and pt_raytrace_render_sharc rebuilds its per-round argument blocks and its captured frame graph at every switch (one
 * small upload, one stream synchronisation, one capture) -- meant for A/B comparison, not for a frame loop; give each form a context. */
int pt_raytrace_render_sharc(PtContext* ctx, const PtTextures* textures);
int pt_sharc_reset(PtContext* ctx);         /* empties the cache (App.cpp:682-685) */
/* the live entries of the resolved buffer, in slot order; *out_count = how many there are. Synchronises. */
int pt_sharc_download(PtContext* ctx, PtSHARCEntry* host_dst, uint32_t capacity, uint32_t* out_count);
/* Test aids (host arrays; they synchronise). Keys: key, level and voxel size of n points (xyz) with normals, camera = the context's.
 * Query: the query decision against the resolved buffer. Update paths: the vertex log of the last update pass rendered with
 * PT_DEBUG_SHARC_LOG_PATHS, path-major, *out_bounces entries per path ((W / f) * (H / f) paths, row-major). */
int pt_sharc_debug_keys(PtContext* ctx, const float* positions, const float* normals, uint32_t n, uint64_t* keys, uint32_t* levels, float* voxel_sizes);
int pt_sharc_debug_query(PtContext* ctx, const float* positions, const float* normals, const float* distances, const float* previous_roughness,
                         uint32_t n, PtSHARCQueryResult* results);
int pt_sharc_download_update_paths(PtContext* ctx, PtSHARCPathVertex* host_dst, uint32_t capacity, uint32_t* out_paths, uint32_t* out_bounces);
int pt_sharc_download_update_scatter(PtContext* ctx, PtSHARCPathScatter* host_dst, uint32_t capacity, uint32_t* out_paths, uint32_t* out_bounces);

/* Measurement (no reference counterpart). Counters cover the work enqueued since the last reset;
 * reading them synchronises the stream. */
typedef struct PtCounters {
    uint64_t PrimaryRays;         /* rays cast by pt_gbuffer_render */
    uint64_t SecondaryRays;       /* rays cast by pt_raytrace_render (bounce rays actually traced) */
    uint64_t NodesVisited;        /* BVH node fetches   (only with PT_DEBUG_TRAVERSAL_STATS) */
    uint64_t TrianglesTested;     /* triangle tests     (only with PT_DEBUG_TRAVERSAL_STATS) */
    uint64_t WavefrontIterations; /* extend/shade rounds launched by the last pt_raytrace_render */
    uint64_t BvhMismatches;       /* PT_DEBUG_BRUTE_FORCE: rays whose BVH result differed from brute force (must be 0) */
    uint64_t StackOverflows;      /* traversal-stack pushes refused for lack of room (must be 0: the builders reject structures that are too deep) */
    uint64_t MaxNodesPerRay;      /* PT_DEBUG_TRAVERSAL_STATS, scenes beyond LDS: node visits of the longest ray */
} PtCounters;
int  pt_reset_counters(PtContext* ctx);
int  pt_get_counters(PtContext* ctx, PtCounters* out);
#define PT_DEBUG_TRAVERSAL_STATS 0x1u
#define PT_DEBUG_TRAVERSAL_V1   0x4u     /* bounce rays use the interleaved TLAS/BLAS traversal of k_gbuffer instead of the phase-aligned one */
#define PT_DEBUG_TRAVERSAL_PHASED 0x8u  /* bounce rays: the TLAS-walking phase-aligned schedule even when the scene is small enough for the flat one */
#define PT_DEBUG_UNFUSED_ROUNDS  0x10u    /* a round = k_shade + k_extend2 (two launches, hit records through HBM) instead of the fused k_round */
#define PT_DEBUG_LOCKSTEP        0x20u    /* scenes too large for LDS: the lock-step schedules (one tile of rays per wave) instead of the streaming form */
#define PT_DEBUG_GATHER_LOCAL_ONLY 0x40u  /* pt_gather_bands places the root's own bands and exchanges nothing: lets ONE GPU play every rank in turn (tests) */
#define PT_DEBUG_BRUTE_FORCE     0x2u     /* bounce rays test every triangle of every instance (validates the LBVH) */
#define PT_DEBUG_GATHER_SELF_EXCHANGE 0x80u /* pt_gather_bands with a world-size-1 communicator: the rank's own bands travel by ncclSend to itself + ncclRecv from
                                             itself (one pair per band, one group) into the full frame -- the grouped p2p path of a real gather on ONE GPU (tests, bench --rehearse-collective) */
#define PT_DEBUG_SHARC_LOG_PATHS 0x100u   /* pt_raytrace_render_sharc keeps the update pass's vertex log (pt_sharc_download_update_paths) */
#define PT_DEBUG_SHARC_SKIP_UPDATE 0x200u /* pt_raytrace_render_sharc skips the update and resolve passes: the query sees the cache as it is */
#define PT_DEBUG_GENERIC_SCENE  0x400u   /* the kernels keep the alpha test and the transmission lobe even when the scene has no non-opaque geometry / no transmissive
                                            material (the library compiles both out of such a scene's frames; the image is the same either way: A/B runs, tests).
                                            pt_bsdf_sample runs the two-branch BSDFSample::Sample under it instead of the merged one of such frames: the same results */
int  pt_set_debug_flags(PtContext* ctx, uint32_t flags);
/* first mismatching ray under PT_DEBUG_BRUTE_FORCE: o.xyz tmin d.xyz tmax | bvh inst slot t - | brute inst slot t - */
int  pt_debug_read_mismatch(PtContext* ctx, float* out16);

/* Developer / test aid: the traversal copy of the scene (8-wide nodes of the top level and of every bottom level, triangle packets in node order,
 * their vertex indices, the instance records in API order and again in top-level leaf order, then -- after LeafInstanceOffset16 + 9 units per
 * instance -- the entry records of the streaming traversal: transform, bases and a copy of the bottom level's root node) copied to host memory,
 * with its section offsets in 16-byte units. tests/ decode it to check the structural invariants of the builder (containment, reference ranges, depth). Synchronises. */
typedef struct PtBlobLayout {
    uint32_t InstanceOffset16, NodeOffset16, TriangleOffset16, LeafInstanceOffset16;
    uint32_t InstanceCount, NodeCount, TriangleCount, Bytes;
} PtBlobLayout;
int  pt_debug_download_blob(PtContext* ctx, void* host_dst, uint64_t capacity_bytes, PtBlobLayout* out_layout);
/* Developer aid: one closest-hit ray through the one-lane two-level walk with a step log of (code, a, b, stack depth) words:
 * 1 enter instance a | 2 triangle b of instance a | 3 node group (a, b) about to be visited | 4 groups after the visit |
 * 5 popped (a, b) | 6 top-level state restored | 7 result (instance, triangle slot). Synchronises. */
int  pt_debug_trace_ray(PtContext* ctx, const PtRayDesc* host_ray, uint32_t* host_log, uint32_t log_words);
/* Test / developer aid: the closest hit of every ray of a batch, through the one-lane two-level walk -- or, while PT_DEBUG_BRUTE_FORCE is set,
 * through every triangle of every instance with no box test in front of the triangle test. The closest-hit rule of the renderer: t in
 * (TMin, TMax) exclusive, no face culling, ties on t to the lowest (instance, geometry, primitive). A miss has Instance = ~0u and T = TMax.
 * U weights vertex 1, V vertex 2; Slot is the triangle packet inside its bottom level. Refused pushes are counted in StackOverflows.
 * Enqueued on the context's stream like pt_trace_visibility. */
typedef struct PtClosestHit { float T, U, V; uint32_t Instance, Geometry, Primitive, Slot, _pad; } PtClosestHit;   /* 32 B */
int  pt_debug_trace_closest(PtContext* ctx, const PtRayDesc* device_rays, uint32_t count, PtClosestHit* device_hits);

/* Per-kernel timing with HIP events recorded on the context stream around every extend / shade launch
 * issued after pt_enable_kernel_timing(ctx, 1); the getter synchronises and returns the sums since then. */
int  pt_enable_kernel_timing(PtContext* ctx, int enable);
int  pt_get_kernel_timing(PtContext* ctx, float* extend_ms, float* shade_ms, uint32_t* extend_launches, uint32_t* shade_launches);
/* the same for the fused round kernel (the default form of a round: trace + shade in one launch) */
int  pt_get_round_timing(PtContext* ctx, float* round_ms, uint32_t* round_launches);

#ifdef __cplusplus
}
#endif
#endif /* PTAMD_H */
