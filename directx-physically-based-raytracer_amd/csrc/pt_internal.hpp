// pt_internal.hpp -- host-side context and the internal interfaces between the .hip files.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <map>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/ptamd.h"
#include "pt_memory.hpp"
#include "pt_trace2.hpp"
#include "pt_sharc.hpp"

namespace pt {

struct WideHeader { uint32_t nodeCount, itemCount, depth, error; };      // written by the collapse kernel

// Device buffers of one tree build. A bottom level built with PT_BUILD_FLAG_ALLOW_UPDATE and the top level keep them, so that a
// refit / rebuild allocates nothing; a static bottom level frees them after the build.
struct TreeBuffers {
    DeviceBuffer<float4> boxLo, boxHi; DeviceBuffer<uint32_t> bounds;
    DeviceBuffer<uint64_t> keys, keysSorted; DeviceBuffer<uint32_t> index, indexSorted;
    DeviceBuffer<uint8_t> sortTemp; size_t sortTempBytes = 0;
    DeviceBuffer<uint64_t> leafKeys; DeviceBuffer<float4> leafLo, leafHi;
    DeviceBuffer<int2> children; DeviceBuffer<int> parentInternal, parentLeaf;
    DeviceBuffer<float4> nodeLo, nodeHi; DeviceBuffer<uint32_t> arrival;
    DeviceBuffer<int> binaryRootOf, slotRefs; DeviceBuffer<uint32_t> leafDst, slotOfPrim;
    DeviceBuffer<WideHeader> header; DeviceBuffer<uint8_t> collapseState;
    DeviceBuffer<uint8_t> dp;                       // collapse cost tables per binary node
};

// wide nodes a tree of nleaves leaves can need. A wide node absorbs at least one binary internal node (nleaves - 1 of them), and no more
// when the cost tables see no gain in opening a child (zero-area subtrees: degenerate triangles, instances of empty meshes): the worst
// case is one wide node per binary node. Typical trees use ~0.13 nodes per leaf; a static bottom level gives the rest back after its build.
inline uint32_t wide_node_capacity(uint32_t nleaves) { return nleaves + 1u; }

struct Blas {
    DeviceBuffer<WideNode> nodes;
    DeviceBuffer<TriPacket> tris;            // node order: the triangles of a node's leaf slots are contiguous
    DeviceBuffer<uint4> idx;                 // the three vertex indices of every triangle, same order (hit reconstruction: no index-buffer hop)
    DeviceBuffer<float> rootBounds;          // lo.xyz hi.xyz
    uint32_t triCount = 0, leafCount = 0, nodeCount = 0, depth = 0, geometryCount = 0;
    bool buildError = false, updatable = false;
    bool hasNonOpaque = true;                // a geometry of the last build / update lacks PT_GEOMETRY_FLAG_OPAQUE
    // a static bottom level lives in the context's traversal copy only, once a top-level build has seen it (pt_api.hip pt_build_top_level):
    // nodes / tris / idx above are empty then, and these are the byte offsets of its three pieces in that copy
    bool inBlob = false; uint64_t blobNodeAt = 0, blobTriAt = 0, blobIdxAt = 0;
    TreeBuffers tree;                        // kept only when updatable
};

// the top level a context builds (its buffers are grow-only)
struct Tlas {
    DeviceBuffer<WideNode> nodes;            // capacity wide_node_capacity(instance capacity)
    DeviceBuffer<float> rootBounds;
    DeviceBuffer<InstanceRecord> instances;  // indexed by InstanceIndex
    DeviceBuffer<const float*> blasBounds;   // per instance: root bounds of its BLAS
    TreeBuffers tree;
};

// host -> device inputs of a top-level build, one upload per build
struct InstanceSource { float transform[12]; uint32_t instanceID, mask, blasSlot, _pad; };
struct BlasEntry { const WideNode* nodes; const TriPacket* tris; const float* rootBounds; uint32_t triCount, nodeCount, nodeBase, triBase; const uint4* idx;
                   uint32_t objectBase, geometryCount; };   // InstanceID of the first instance that refers to the bottom level: ObjectData[objectBase + geometry] describes its meshes
struct BlobCopy { const void* src; void* dst; uint64_t n16; };

// What a render reads of the scene: views of the storage of the context that built the top level -- this one, or the one it views
// (pt_share_scene). Written when a top-level build commits, copied by pt_share_scene, cleared by drop_tlas and by the destruction of a viewed
// owner. Nothing here is freed through these pointers.
struct SceneRefs {
    const InstanceRecord* instances = nullptr; uint32_t instanceCount = 0;
    uint64_t triangleCount = 0;              // sum over instances
    BlobView blob{};                         // compact traversal copy of TLAS + instances + every referenced BLAS
    const BlasEntry* blasTable = nullptr; uint32_t blasTableCount = 0, blasTableMaxTris = 0;   // the top-level build's table of bottom levels
    const InstanceSource* instSource = nullptr;
    // A candidate can be non-opaque: some geometry of a bottom level this top level refers to lacks PT_GEOMETRY_FLAG_OPAQUE (the only source
    // include/ptamd.h has: no instance flags, no ray flags on closest-hit rays). Unknown -- no top level -- is "has".
    bool hasNonOpaque = true;
};

// What hit reconstruction needs of an object's geometry, resolved once per change of (ObjectData, heap) by the validation kernel: the
// object record -> descriptor table -> buffer chain of the reference (RaytracingHelpers.hlsli:82-85) is one fetch here.
struct alignas(16) ShadeGeom { const uint8_t* vb; uint32_t stride, nOff, tOff, uvOff[2], _pad; };   // offsets of normal / tangent / the two texture-coordinate sets inside a vertex; ~0u: attribute absent.
                                                                                                 // (a triangle's vertex indices come from the traversal copy, not from the object's index buffer)
static_assert(sizeof(ShadeGeom) == 32, "layout");

// everything a render kernel needs about the scene, passed by value as a kernel argument
struct SceneView {
    AccelView accel;
    const PtObjectData* objects;
    const ShadeGeom* shadeGeom;              // [objectCount]
    const HeapEntry* shadeTex;               // [objectCount * 7]: the objects' resolved texture slots (pt_texture.hpp TextureSlots)
    const PtInstanceData* instanceData;
    const HeapEntry* heap;
    const float* srgbLut;                    // 256-entry sRGB -> linear table (device)
    uint32_t objectCount, heapCount;
};

struct FrameView {                           // G-buffer geometry of this context's shard
    uint32_t width, height;                  // full frame
    uint32_t localRows;                      // rows held by this rank
    uint32_t rankIndex, rankCount, bandHeight;
};

// wavefront path state, structure of arrays, 16-byte records (DESIGN.md "Queues")
struct PathQueue {
    float4* s0;      // throughput.xyz | pixel (local index, bits)
    float4* s1;      // sampleRadiance.xyz | rng state (bits)
    float4* s2;      // radiance sum.xyz | sample << 16 | bounce << 1 | fresh (bits)
    float4* r0;      // ray origin.xyz | tmin
    float4* r1;      // ray direction.xyz | tmax
    uint4*  hit;     // instance | triangle slot in the BLAS | u bits | v bits      (instance ~0u = miss)
};

// Queue geometry (pt_kernels.hip "wavefront path tracer"): the path queue is cut into independent sub-queues
// How many: a power of two chosen per frame by the form that renders it (FramePlan::sqShift = its log2). The fused round kernel likes 32 (C2: 64 -0.4 %,
// 128 -0.9 %), the streaming form 128 (C5 +3 %, C3 +0.5 % over 32; 256 the same, 512 less): a sub-queue is then shared by 16 waves instead of 64,
// cursors are less contended and run dry at a finer grain. Per round the counters are: entries traced | fresh | cursor of the streaming form,
// one word per sub-queue each (3 << sqShift words).
constexpr uint32_t kSubQueueShiftFused = 5, kSubQueueShiftStream = 7, kSubQueuesMax = 1u << kSubQueueShiftStream;

struct FrameConstants { PtCamera cam; PtSceneData sd; PtGraphicsSettings gs; };
struct RoundArgs;

// ---- animation (pt_anim.hip). What the posing kernel reads of a rig and of an animated object: device pointers into the one device buffer
// each of them owns. Written once, at creation.
struct AnimRigView {
    const int* parents; const float* rest;           // [nodes] | [nodes * 10]: T3 R4 S3
    const uint32_t* levelNodes; const uint32_t* levelStart;   // the nodes ordered by depth | [levels + 1] into levelNodes
    const uint2* channels;                           // [clips * nodes * 3] {FirstKey, KeyCount}
    const float* keyTimes; const float4* keyValues;
    uint32_t nodeCount, levelCount, clipCount, _pad;
};
struct AnimObjectView {
    AnimRigView rig;
    float transform[16];                             // RenderObject.Transform()
    float* globals;                                  // [nodes * 16]
    float* skeletal;                                 // [joints of all skins * 12]
    float* skinInverse;                              // [skins * 16]: Global(meshNode)^-1 of this evaluation
    const uint32_t* bindingNodes; const uint32_t* bindingInstances; const float* bindingGlobals;
    const uint32_t* skinMeshNodes;                   // [skins]: the rig node of each skinned mesh node
    const uint32_t* jointNodes; const uint32_t* jointSkin; const float* inverseBinds;   // [joints of all skins]: rig node | skin | InverseBind
    uint32_t bindingCount, skinCount, jointCount, _pad;
};
struct AnimStateDev { const AnimObjectView* object; uint32_t clip, first; double time; };   // one per state of pt_anim_evaluate
struct AnimRig { DeviceBuffer<uint8_t> dev; AnimRigView view{}; std::vector<double> durations; uint32_t users = 0; };
struct AnimObject {
    uint64_t rig = 0;
    DeviceBuffer<uint8_t> dev; const AnimObjectView* viewDev = nullptr;
    float* globals = nullptr; float* skeletal = nullptr;
    uint32_t nodeCount = 0, maxInstance = 0; bool hasBindings = false;
    std::vector<uint32_t> skinFirstJoint;
    bool evaluated = false;                          // PreviousObjectToWorld of the first evaluation = its ObjectToWorld
    uint64_t stamp = 0;                              // the evaluate call that last named it (an object twice in one call is refused)
};

struct DeviceCounters {
    unsigned long long primaryRays, secondaryRays, nodesVisited, trianglesTested;
    unsigned int mismatchCount, stackOverflows;   // PT_DEBUG_BRUTE_FORCE: rays whose BVH result differs from brute force | refused stack pushes (must be 0)
    float mismatchRay[16];                   // first such ray: o.xyz tmin d.xyz tmax | bvh inst slot t - | brute inst slot t -
    unsigned int maxNodesPerRay, _pad2;      // PT_DEBUG_TRAVERSAL_STATS, streaming traversal: the longest walk
};

// What each of the three screen-space filters (pt_filter.hpp) keeps between calls, beside its settings and its history buffers.
struct FilterState {
    bool have = false;                       // pt_*_set_constants has accepted settings
    uint32_t parity = 0;                     // which half of each ping-pong pair of the history the last call wrote
    uint64_t frames = 0;                     // calls since the history was last reset; 0: the next call finds none
    uint32_t size[4] = {0, 0, 0, 0};         // the frame the history was laid out for by the last call: w, h (and the output's w, h)
    void advance(uint32_t w, uint32_t h, uint32_t ow = 0, uint32_t oh = 0) { parity ^= 1u; frames += 1; size[0] = w; size[1] = h; size[2] = ow; size[3] = oh; }
    uint32_t shown(int k) const { return frames != 0 ? size[k] : 0u; }   // after a reset there is no history to show: 0 x 0
};

struct Context {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string lastError;

    std::vector<HeapEntry> heapHost;
    DeviceBuffer<HeapEntry> heapDev; bool heapDirty = true;
    DeviceBuffer<float> srgbLutDev;
    bool heapHasTextures = false;             // any Texture2D / TextureCube descriptor: selects the TEXTURED kernel variants

    std::map<uint64_t, Blas> blas; uint64_t nextBlasId = 1;
    TreeBuffers buildScratch;                         // build buffers of static bottom levels, reused from build to build (grow-only)
    Tlas tlas; bool haveTlas = false;
    DeviceBuffer<uint8_t> blobDev;                    // this context's traversal copy (SceneRefs::blob views it once a top-level build commits)
    SceneRefs scene;                                  // what renders read: views of this context's top level, or of sceneOwner's
    Context* sceneOwner = nullptr;                    // pt_share_scene: the context whose scene `scene` views
    std::vector<Context*> viewers;                    // contexts viewing THIS context's scene (pt_destroy of a viewed owner detaches them)
    uint32_t framesInFlight = 1;                      // pt_set_frames_in_flight: how many contexts render concurrently on this GPU (grid sizing)
    std::vector<uint64_t> tlasBlasIds;                // bottom levels the live TLAS refers to (pt_release_bottom_level checks)
    std::vector<uint8_t> tlasUploadHost; DeviceBuffer<uint8_t> tlasUploadDev;   // InstanceSource | BlasEntry | BlobCopy
    struct UploadStage { PinnedBuffer<uint8_t> host; Event event; };  // pinned staging of that upload, two in turn
    UploadStage tlasStage[2]; uint32_t tlasStageNext = 0;
    PinnedBuffer<WideHeader> tlasHeaderHost; Event tlasHeaderEvent; bool tlasHeaderPending = false;   // lazy depth / error check
    uint32_t maxBlasDepth = 0, tlasNodeReserve = 0;   // tlasNodeReserve: top-level nodes reserved at the head of the traversal copy by the last build
    uint32_t tlasValidatedCount = ~0u, persistentGrid = 0;
    uint64_t tlasBindingHash = 0;                     // over (InstanceID, bottom-level id) of the instances, in order: what the shared-geometry check depends on
    uint64_t tlasObjectEnd = 0;                       // max over instances of InstanceID + geometry count: ObjectData must reach that far
    DeviceBuffer<ShadeGeom> shadeGeomDev;             // per object
    DeviceBuffer<HeapEntry> shadeTexDev;              // 7 resolved texture slots per object
    // per-frame copy of the vertex normals, one record per triangle packet of the traversal copy (pt_shade.hpp ShadeTables)
    DeviceBuffer<uint4> shadeRecA; DeviceBuffer<uint32_t> shadeRecB;
    bool normalsShared = false;              // every instance of a bottom level resolves to the same vertex buffer / stride / normal offset (checked with the objects)
    bool sharedVerdict = false;              // what the last shared-geometry check said (normalsShared is put aside while there is no top level)
    bool validated = false; DeviceBuffer<uint32_t> validateDev;   // descriptor / index validation of the scene inputs (pt_api.hip make_views)
    const void* validatedObjects = nullptr; uint32_t validatedObjectCount = 0;
    // Scene facts behind the kernels' ALPHA / TRANSMISSION switches (plan_frame); unknown is "has". hasTransmission: some object has Material.Transmission != 0
    // or a Transmission texture (k_validate_objects, with the validation: per change of ObjectData / heap / top level, and after pt_invalidate_object_data).
    // gbufferTransmission: the same fact when this context last rendered a G-buffer -- bounce 0 reads Transmission from there, not from ObjectData.
    bool hasTransmission = true, gbufferTransmission = true;

    PtCamera camera{}; PtSceneData sceneData{}; PtGraphicsSettings settings{};
    bool haveCamera = false, haveSceneData = false, haveSettings = false;
    const PtObjectData* objects = nullptr; uint32_t objectCount = 0;
    const PtInstanceData* instanceData = nullptr; uint32_t instanceDataCount = 0;
    PtSharding sharding{0, 1, 16, 0};

    DeviceBuffer<uint4> queueArrays[2][6];            // s0 s1 s2 r0 r1 hit of each path queue, 16 B per entry
    PathQueue queue[2]{};                             // ... as the kernels take them
    DeviceBuffer<uint4> primaryRecords;               // 48 B per local pixel: the primary surface as bounce 0 reads it (k_pt_init)
    DeviceBuffer<float2> pixelAux;                    // denoiser modes: first-bounce hit distance | isDiffuse per pixel
    DeviceBuffer<FrameConstants> frameConstants;
    GraphExec graphExec; std::string graphKey; bool disableGraphs = false;
    // chains of a frame (pt_kernels.hip launch_raytrace): the rounds of a group of sub-queues need nothing from the other groups, so each group's
    // chain of launches is a linear graph replayed on a stream of its own, behind the frame's preamble and joined to the context's stream.
    static constexpr uint32_t kMaxChains = 4;
    uint32_t chains = 0;                              // 0: the library chooses (pt_set_round_chains)
    Stream chainStream[kMaxChains - 1]; Event chainFork, chainJoin[kMaxChains - 1];
    GraphExec chainGraph[kMaxChains]; std::string chainGraphKey;
    DeviceBuffer<uint32_t> queueCounts;
    DeviceBuffer<RoundArgs> roundArgs; std::string roundArgsKey;   // per-round argument blocks of k_round
    DeviceBuffer<DeviceCounters> counters;
    uint64_t lastIterations = 0;
    uint32_t debugFlags = 0;

    void* comm = nullptr; bool commOwned = false; uint32_t commRank = 0, commWorld = 1;   // ncclComm_t of pt_gather_bands (pt_comm.hip)

    bool timing = false;
    std::vector<Event> evExtend, evShade, evRound;     // begin/end pairs since timing was enabled
    uint32_t nExtend = 0, nShade = 0, nRound = 0;

    // direct lighting (pt_di.hip): per context. A context that views another's scene (pt_share_scene) lists its emissive triangles from the owner's
    // read-only top-level inputs into a list of its own; the per-render records and the sampling table are the context's too.
    PtDISettings diSettings{}; bool haveDISettings = false;
    uint64_t tlasLightHash = 0;                       // over (InstanceID, InstanceMask, bottom-level id) of the top level's instances, in order
    uint32_t objectDataGen = 0;                       // bumped by pt_invalidate_object_data
    DeviceBuffer<uint4> lightList; uint32_t lightCount = 0;     // (instance, geometry, primitive, object) per emissive triangle
    DeviceBuffer<uint32_t> lightInstStart;                      // per instance: first list entry; [instanceCount]: the total
    uint64_t lightListKey = 0; bool lightListValid = false;
    DeviceBuffer<PtTriangleLight> lightRecords; DeviceBuffer<float> lightCdf, lightBlockSums; uint32_t lightRecordCount = 0;   // lightCdf: cdf | powers
    // reservoir reuse (pt_di_set_resampling): A = temporal output, B = final reservoirs = next frame's history
    PtDIResamplingSettings diReuse{}; bool diReuseOn = false;
    DeviceBuffer<PtDIReservoir> diResA, diResB;
    DeviceBuffer<int8_t> diOffsets;                   // the spatial neighbour-offset table, 8192 (x, y) pairs
    bool diHistoryValid = false; uint32_t diHistorySize[2] = {0, 0}; uint64_t diHistoryLightKey = 0; uint32_t diResCount = 0;
    // local-light sampling (pt_di_set_light_sampling): the Power_RIS tiles and the ReGIR cells of the last render, per context
    PtDIVisibilitySettings diVisibility{}; bool diVisibilityOn = false;   // pt_di_set_visibility: any flag set
    PtDIPairwiseSettings diPairwise{};                                      // pt_di_set_pairwise
    PtDILightSamplingSettings diSampling{};
    DeviceBuffer<PtDIPresampledLight> diTiles, diCells;
    uint32_t diTileCount = 0, diCellCount = 0;        // entries the last render filled (0: not filled)
    uint32_t diBrdfCount = 0;                         // ... and BRDF candidate records (diBrdfRecords below)
    uint32_t diReGIRLayout = 0;                       // pt_di_set_regir_layout: PT_DI_REGIR_LAYOUT_*
    DeviceBuffer<float> diOnion;                      // the Onion layout's tables (OnionTables), uploaded by the first Onion render
    // BRDF candidates (pt_di_set_brdf_sampling): lightFirst[object] = the first list entry of an emissive object (~0u: not emissive), built with
    // the light list; diBrdfRecords: the last render's candidates, BrdfSamples per local pixel
    struct DIBrdfSettings { uint32_t BrdfSamples = 0; float BrdfCutoff = 0.0f; } diBrdf;
    DeviceBuffer<uint32_t> lightFirst;
    DeviceBuffer<uint4> diBrdfRecords;                // (li | ~0u, U, V, pdf of the ray)
    // the local-light PDF texture (pt_di_set_pdf_mipmap): every level of the chain in one grow-only allocation, level 0 first, and behind the
    // last level one float, top * M * M (what a.total points at while the setting acts). diPdfSize: the last render's (width, height, mips); 0: none
    uint32_t diPdfMipmap = 0;
    DeviceBuffer<float> diPdfTexture;
    uint32_t diPdfSize[3] = {0, 0, 0};

    // animation (pt_anim.hip): rigs, animated objects, and the staging of pt_anim_evaluate's states (a pinned ring guarded by events, like
    // tlasStage; the device array is grow-only)
    std::map<uint64_t, AnimRig> animRigs; std::map<uint64_t, AnimObject> animObjects; uint64_t nextAnimId = 1, animStamp = 0;
    UploadStage animStage[2]; uint32_t animStageNext = 0;
    DeviceBuffer<AnimStateDev> animStatesDev;

    // post-processing (pt_post.hip): one slot per bloom stage, each the size of the level it writes (the bytes of the reference's two pyramids)
    PtPostProcessSettings post{}; bool havePost = false;
    DeviceBuffer<ushort4> postLevels;
    uint32_t postDims[9][2] = {};                     // what each stage wrote in the last render with bloom on; 0 x 0: not written
    size_t postOffset[9] = {};                        // texel offset of each stage's slot in postLevels

    // denoiser (pt_denoise.hip): every per-pixel array of the history in one grow-only allocation, 17 float4 per pixel of the frame (the
    // ping-pong pairs of the accumulated colours, moments and guide records, the a-trous work buffers, the lengths and variances)
    PtDenoiserSettings dn{}; FilterState dnState;     // size: the frame of the last pt_denoiser_process
    DeviceBuffer<float4> dnHistory;

    // upscaler (pt_upscale.hip): the history in one grow-only allocation, per output pixel two parities of a float4 (the colour in the
    // tone-mapped space and the accumulated weight n) and, behind them, two parities of the depth: 40 B
    PtUpscalerSettings up{}; FilterState upState;     // size: the output frame of the last pt_upscaler_process
    DeviceBuffer<float4> upHistory;

    // ray reconstruction (pt_reconstruct.hip): two grow-only allocations. rrHistory, per render pixel ten float4 (two parities of the
    // signal with its length and of the two guide records, the albedo, the a-trous ping-pong, two parities of the moments): 160 B.
    // rrOutput, per output pixel two parities of a float4 (tone-mapped colour, n) and of the depth: 40 B. It shares nothing with the upscaler.
    PtReconstructionSettings rr{}; FilterState rrState;   // size: render w, h and output w, h of the last pt_reconstruction_process
    DeviceBuffer<float4> rrHistory, rrOutput;
    uint32_t rrFinal = 0;                             // which a-trous work buffer holds the last call's filtered signal

    // frame generation (pt_framegen.hip): four grow-only allocations. The previous frame's Color (8 B per output pixel) and LinearDepth (4 B
    // per render pixel), the midpoint field of the last call (8 B per render pixel), the class bytes of the test aid (1 B per output pixel).
    // fgState.frames == 0: there is no previous frame; fgState.parity is not used (the previous frame is an explicit copy).
    PtFrameGenerationSettings fg{}; FilterState fgState;  // size: render w, h and output w, h of the last call that generated a frame
    DeviceBuffer<uint64_t> fgPrevColor, fgField;
    DeviceBuffer<float> fgPrevDepth;
    DeviceBuffer<uint8_t> fgClass;
    float fgPrevJitter[2] = { 0.0f, 0.0f };           // the Camera.Jitter of the frame in fgPrevDepth
    bool fgFieldValid = false;                        // the last call generated a frame: field and class bytes are its

    // sharpening (pt_sharpen.hip): the settings alone; the pass has no history and no memory of its own (shState.have is all it uses)
    PtSharpenSettings sh{}; FilterState shState;

    // SHARC radiance cache (pt_sharc.hip): per context, also for a context that views another's scene. sharcVoxels[sharcParity] is VoxelData (this
    // frame's deposits, then the resolved cache), the other one PreviousVoxelData; they swap after the query.
    PtSHARCSettings sharcSettings{}; bool haveSharcSettings = false;
    uint32_t sharcCapacity = 0, sharcParity = 0;      // capacity 0: not configured
    DeviceBuffer<unsigned long long> sharcKeys;       // HashEntries
    DeviceBuffer<uint4> sharcVoxels[2];
    DeviceBuffer<SharcView> sharcView;                // what the query kernels read, rewritten per render in stream order
    DeviceBuffer<float> sharcRough[2];                // previousRoughness of the two path queues' entries (allocated by the first SHARC render)
    DeviceBuffer<PtSHARCPathScatter> sharcLogScatter;
    DeviceBuffer<PtSHARCPathVertex> sharcLog; uint32_t sharcLogPaths = 0, sharcLogBounces = 0;   // PT_DEBUG_SHARC_LOG_PATHS: the last update pass's vertices
};

// ---- API plumbing shared by the files of the C ABI (defined in pt_api.hip) ------------------------------------------------------------
std::string& create_error();             // the message pt_last_error(NULL) returns (errors of the context-free entry points)
int fail(Context* c, int status, const std::string& msg);       // records msg in the context (null: in create_error()) and returns status
int fail_hip(Context* c, hipError_t e, const char* what);
#define API_HIP(ctx, expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return pt::fail_hip(ctx, e_, #expr); } while (0)
#define API_ARG(ctx, cond, msg) do { if (!(cond)) return pt::fail(ctx, PT_ERROR_INVALID_ARGUMENT, msg); } while (0)
// the view set-up of every render operator: waits for the top-level build's verdict, uploads the heap, validates the scene inputs
int make_views(Context& c, uint32_t width, uint32_t height, SceneView& sv, FrameView& fv, bool needFrameInputs = true);
// what pt_raytrace_render and pt_raytrace_render_sharc check alike, behind their own checks: settings ranges and texture bindings
int check_raytrace_args(Context& c, const PtTextures* tx);
// pt_mipmap_generate behind its context checks (pt_mip.hip): levels is a host array of device pointers; the DI pass builds its PDF texture's chain with it
int mip_generate(Context& c, float* const* levels, uint32_t width, uint32_t height, uint32_t mips);
// false for a rank of the sharding that holds no row of a width x height frame (or for an empty frame): no texture binding is asked of it
bool rank_holds_pixels(const Context& c, uint32_t width, uint32_t height);

// The tail of a counted download (pt_*_download_*): the counts of what the last render left go out -- `count` rows of `row` records -- then
// min(capacity, count * row) records. Synchronises.
template <typename T>
int download_counted(Context& c, const T* src, uint32_t count, uint32_t row, T* host_dst, uint32_t capacity, uint32_t* out_count, uint32_t* out_row = nullptr)
{
    API_HIP(&c, hipSetDevice(c.device));
    API_HIP(&c, hipStreamSynchronize(c.stream));
    *out_count = count;
    if (out_row) *out_row = row;
    const size_t n = std::min((size_t)capacity, (size_t)count * row);
    if (n) API_HIP(&c, hipMemcpy(host_dst, src, sizeof(T) * n, hipMemcpyDeviceToHost));
    return PT_OK;
}

// Run-time flags -> template arguments: with_flags(f, a, b, ...) calls the generic lambda f with one std::bool_constant per flag, so a
// kernel launch is written once and instantiated for every combination of its switches.
template <typename F> void with_flags(F&& f) { f(); }
template <typename F, typename... Rest> void with_flags(F&& f, bool first, Rest... rest)
{
    if (first) with_flags([&](auto... bs) { f(std::true_type{}, bs...); }, rest...);
    else with_flags([&](auto... bs) { f(std::false_type{}, bs...); }, rest...);
}

// Developer builds (tools/ab.sh): -DPT_SPEC_FORCE_ALPHA / -DPT_SPEC_FORCE_TRANSMISSION hold one of the two scene switches at "has" whatever the scene,
// and -DPT_SPEC_SPLIT gives k_round the two switches apart, so that each can be timed alone. The product defines none of them.
#ifdef PT_SPEC_FORCE_ALPHA
constexpr bool kSpecForceAlpha = true;
#else
constexpr bool kSpecForceAlpha = false;
#endif
#ifdef PT_SPEC_FORCE_TRANSMISSION
constexpr bool kSpecForceTransmission = true;
#else
constexpr bool kSpecForceTransmission = false;
#endif
#ifdef PT_SPEC_SPLIT
constexpr bool kSpecSplit = true;
#else
constexpr bool kSpecSplit = false;
#endif

// Developer builds (tools/ab.sh): -DPT_PLAIN_NO_MERGED gives the untextured plain form of k_round (no alpha test, no third lobe) the two-branch
// BSDFSample::Sample back, so that the merged form can be timed against it. The product does not define it.
#ifdef PT_PLAIN_NO_MERGED
constexpr bool kPlainMerged = false;
#else
constexpr bool kPlainMerged = true;
#endif

// pt_bvh.hip
hipError_t build_blas_device(const PtGeometryDesc* geoms, uint32_t ngeoms, bool allowUpdate, hipStream_t stream, Blas& out);
hipError_t refit_blas_device(const PtGeometryDesc* geoms, uint32_t ngeoms, hipStream_t stream, Blas& b);
hipError_t build_tlas_prepare(Tlas& out, uint32_t n);
hipError_t build_tlas_device(const InstanceRecord* dInstances, const float* const* dBlasBounds, uint32_t n, hipStream_t stream, Tlas& out);
hipError_t launch_instance_records(const InstanceSource* src, const BlasEntry* table, uint32_t n, InstanceRecord* rec, const float** bounds, uint32_t* sceneBounds, hipStream_t stream);
hipError_t launch_blob_assembly(const InstanceRecord* inst, const Tlas& tlas, const BlasEntry* table, uint32_t n, InstanceT* outInst,
                                InstanceT* outLeafInst, const BlobCopy* jobs, uint32_t njobs, f4v* outEnter, hipStream_t stream);
__host__ __device__ void invert_3x4(const float m[12], float out[12]);

// pt_anim.hip: src[i].transform <- instances[i].ObjectToWorld for every i whose src[i]._pad is set (pt_build_top_level_posed)
hipError_t launch_patch_instance_sources(hipStream_t stream, InstanceSource* src, const PtInstanceData* instances, uint32_t n);

// pt_skin.hip
hipError_t launch_skin(hipStream_t stream, const void* skeletal, const float* transforms, void* vertices, void* motion, uint32_t count);

// Everything the launches of one path-traced frame depend on, decided once per frame by plan_frame (pt_kernels.hip): the launchers read the
// plan and the context's buffers, and re-derive nothing. Zero-initialised before it is filled: its bytes are part of the graph key.
struct FramePlan {
    uint32_t rounds, segCap, grid, sqShift;          // rounds of the frame | entries per sub-queue segment | persistent grid | log2 of the sub-queues
    bool streaming, fused, first;                    // the form: streaming rounds | fused rounds | k_pt_first (either product form) or k_pt_init + round 0
    bool flat, lds;                                  // lock-step traversal: flat instance scan or phased walk | traversal copy staged in LDS
    uint32_t ldsFixed, roundLds, extend2Lds;         // fixed LDS bytes of the schedule | dynamic LDS bytes of k_round | of k_extend2
    uint32_t objectsInLds, recordsInLds;             // what k_round stages behind the traversal copy
    bool recordsUsable;                              // the frame has normal records (k_capture_normals runs)
    bool writeT, stats, di, textured, sharc;         // the kernel variants' switches
    bool alpha, transmission;                        // ... and the scene's: non-opaque geometry / transmissive materials may exist (both false: compiled out of k_round)
    float2* aux;                                     // denoiser modes: the per-pixel auxiliary record, else null
    uint32_t nsq() const { return 1u << sqShift; }
    uint32_t cstride() const { return 3u * nsq(); }  // traced + fresh counters + the streaming form's cursor, per round
};

// pt_stream.hip
hipError_t launch_shade(Context& c, const FramePlan& p, const SceneView& sv, const FrameView& fv, const PtTextures& tx, uint32_t round, uint32_t grid, hipStream_t stream,
                        uint32_t sqBase, uint32_t sqCount);
hipError_t launch_extend_stream(Context& c, const FramePlan& p, const AlphaContext& ac, uint32_t round, hipStream_t stream, uint32_t sqBase, uint32_t sqCount);

// pt_kernels.hip
hipError_t launch_gbuffer(Context& c, const SceneView& sv, const FrameView& fv, uint32_t flags, const PtTextures& tx);
hipError_t launch_raytrace(Context& c, const SceneView& sv, const FrameView& fv, const PtTextures& tx, bool sharcQuery);
hipError_t launch_visibility(Context& c, const SceneView& sv, const void* rays, uint32_t count, void* out);
hipError_t launch_bsdf_evaluate(hipStream_t stream, const float* q, uint32_t count, float* r);
hipError_t launch_bsdf_sample(hipStream_t stream, const float* q, uint32_t count, float* r, bool merged);   // merged: Sample as the plain k_round runs it
hipError_t launch_debug_trace(Context& c, const SceneView& sv, const float* ray8, uint32_t* devLog, uint32_t logCap);
hipError_t launch_debug_closest(Context& c, const SceneView& sv, const void* rays, uint32_t count, void* hits);
uint32_t round_objects_in_lds(const Context& c, uint32_t objectCount, bool haveShadeGeom);   // the fused round kernel's LDS tables (PtAccelStats)
uint32_t round_records_in_lds(const Context& c, uint32_t objectCount, bool haveShadeGeom);
inline bool normal_records_usable(const Context& c) { return c.normalsShared && c.scene.blasTable && c.scene.blasTableCount <= 65535u /* grid.y of k_capture_normals */ && c.shadeRecB && c.scene.blob.triCount && c.scene.blob.triCount <= c.shadeRecB.capacity(); }
hipError_t launch_check_shared_geometry(hipStream_t stream, const InstanceSource* src, const BlasEntry* table, uint32_t n, const ShadeGeom* shadeGeom, uint32_t* out);
hipError_t launch_validate_objects(hipStream_t stream, const PtObjectData* objects, uint32_t count, const HeapEntry* heap, uint32_t heapCount, uint32_t* out, ShadeGeom* shadeGeom, HeapEntry* shadeTex);
hipError_t launch_deinterleave(hipStream_t stream, void* dst, const void* src, const uint64_t* rankOffsetsHost, uint32_t rankCount,
                               uint32_t bandHeight, uint32_t width, uint32_t height, uint32_t pixelBytes);

} // namespace pt

struct PtContext { pt::Context c; };      // the opaque handle of include/ptamd.h
