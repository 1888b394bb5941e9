// pt_api.hip -- the C ABI of include/ptamd.h: context, descriptor heap, acceleration-structure
// lifecycle, per-frame constants and the two render operators. No exception crosses this file.
#include "pt_internal.hpp"

#include <cmath>
#include <cstdio>
#include <cstring>

using namespace pt;

static thread_local std::string g_createError;
namespace pt { std::string& create_error() { return g_createError; } }

int pt::fail(Context* c, int status, const std::string& msg)
{
    if (c) c->lastError = msg; else g_createError = msg;
    return status;
}
int pt::fail_hip(Context* c, hipError_t e, const char* what)
{
    return fail(c, e == hipErrorOutOfMemory ? PT_ERROR_OUT_OF_MEMORY : PT_ERROR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

static int poll_tlas_header(Context& c, bool wait);

extern "C" {

int pt_abi_version(void) { return PTAMD_ABI_VERSION; }

int pt_create(int device_ordinal, PtContext** out_ctx)
{
    if (!out_ctx) return fail(nullptr, PT_ERROR_INVALID_ARGUMENT, "out_ctx is NULL");
    *out_ctx = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) return fail(nullptr, PT_ERROR_NO_DEVICE, "no HIP device visible: the path tracer has no CPU fallback");
    if (device_ordinal < 0 || device_ordinal >= n) return fail(nullptr, PT_ERROR_INVALID_ARGUMENT, "device ordinal out of range");
    if ((e = hipSetDevice(device_ordinal)) != hipSuccess) return fail_hip(nullptr, e, "hipSetDevice");
    PtContext* p = new (std::nothrow) PtContext();
    if (!p) return fail(nullptr, PT_ERROR_OUT_OF_MEMORY, "host allocation failed");
    p->c.device = device_ordinal;
    if ((e = p->c.counters.reserve(1)) != hipSuccess) { delete p; return fail_hip(nullptr, e, "hipMalloc(counters)"); }
    hipMemset(p->c.counters.data(), 0, sizeof(DeviceCounters));
    *out_ctx = p;
    return PT_OK;
}

static void detach_from_owner(Context& c)
{
    Context* o = c.sceneOwner;
    if (!o) return;
    for (size_t i = 0; i < o->viewers.size(); i++) if (o->viewers[i] == &c) { o->viewers.erase(o->viewers.begin() + i); break; }
    c.sceneOwner = nullptr;
}

static void drop_tlas(Context& c) { c.haveTlas = false; c.tlasBlasIds.clear(); c.scene = SceneRefs{}; c.normalsShared = false; }

// The context is about to give up its traversal copy while it keeps its bottom levels (it becomes a view of another context's scene): the
// adopted ones get arrays of their own again. Each is copied into new arrays first and only then stops living in the copy, so that a
// failure leaves every bottom level whole. Synchronous; a rare path.
static hipError_t materialise_adopted(Context& c)
{
    if (!c.blobDev) return hipSuccess;
    hipError_t e = hipStreamSynchronize(c.stream);
    const uint8_t* blob = c.blobDev.data();
    for (auto& kv : c.blas) {
        Blas& b = kv.second;
        if (!b.inBlob || e != hipSuccess) continue;
        const size_t nt = b.triCount ? b.triCount : 1;
        DeviceBuffer<WideNode> nodes; DeviceBuffer<TriPacket> tris; DeviceBuffer<uint4> idx;
        if ((e = nodes.reserve(b.nodeCount ? b.nodeCount : 1)) != hipSuccess) break;
        if ((e = tris.reserve(nt)) != hipSuccess) break;
        if ((e = idx.reserve(nt)) != hipSuccess) break;
        if ((e = hipMemcpy(nodes.data(), blob + b.blobNodeAt, sizeof(WideNode) * (size_t)b.nodeCount, hipMemcpyDeviceToDevice)) != hipSuccess) break;
        if (b.triCount && (e = hipMemcpy(tris.data(), blob + b.blobTriAt, sizeof(TriPacket) * (size_t)b.triCount, hipMemcpyDeviceToDevice)) != hipSuccess) break;
        if (b.triCount && (e = hipMemcpy(idx.data(), blob + b.blobIdxAt, 16 * (size_t)b.triCount, hipMemcpyDeviceToDevice)) != hipSuccess) break;
        b.nodes = std::move(nodes); b.tris = std::move(tris); b.idx = std::move(idx); b.inBlob = false;
    }
    return e;
}

void pt_destroy(PtContext* ctx)
{
    if (!ctx) return;
    Context& c = ctx->c;
    hipSetDevice(c.device);
    hipStreamSynchronize(c.stream);
    for (const Stream& st : c.chainStream) if (st) hipStreamSynchronize(st.get());   // (the context's stream has waited for them already: every frame joins its chains)
    pt_comm_destroy(ctx);
    // an owner that is still viewed (pt_share_scene): its viewers lose the scene -- their next render answers PT_ERROR_NOT_READY -- after
    // their streams have drained, and never touch this context again
    for (Context* v : c.viewers) {
        hipStreamSynchronize(v->stream);
        v->sceneOwner = nullptr;
        drop_tlas(*v);
        v->objects = nullptr; v->objectCount = 0; v->instanceData = nullptr; v->instanceDataCount = 0;
        v->graphExec.reset(); v->graphKey.clear(); v->chainGraphKey.clear();
    }
    c.viewers.clear();
    detach_from_owner(c);
    delete ctx;                                          // the owners in Context free the rest
}

const char* pt_last_error(const PtContext* ctx) { return ctx ? ctx->c.lastError.c_str() : g_createError.c_str(); }

int pt_set_stream(PtContext* ctx, void* hip_stream)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    ctx->c.stream = (hipStream_t)hip_stream;
    return PT_OK;
}

int pt_set_frames_in_flight(PtContext* ctx, uint32_t frames)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    API_ARG(&ctx->c, frames >= 1, "frames in flight must be at least 1");
    ctx->c.framesInFlight = frames;
    ctx->c.graphKey.clear(); ctx->c.chainGraphKey.clear();   // the launch geometry of the captured frame depends on it
    return PT_OK;
}

int pt_set_round_chains(PtContext* ctx, uint32_t chains)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    API_ARG(&ctx->c, chains <= Context::kMaxChains, "at most 4 chains");
    ctx->c.chains = chains;
    ctx->c.graphKey.clear(); ctx->c.chainGraphKey.clear();
    return PT_OK;
}

int pt_sync(PtContext* ctx)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    API_HIP(&ctx->c, hipSetDevice(ctx->c.device));
    API_HIP(&ctx->c, hipStreamSynchronize(ctx->c.stream));
    return poll_tlas_header(ctx->c, true);
}

// ---- descriptor heap ------------------------------------------------------------------------
int pt_heap_resize(PtContext* ctx, uint32_t descriptor_count)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    ctx->c.heapHost.resize(descriptor_count, HeapEntry{ nullptr, 0, 0, 0 });
    ctx->c.heapDirty = true;
    return PT_OK;
}

int pt_heap_set_buffer(PtContext* ctx, uint32_t descriptor, const void* device_ptr, uint64_t bytes, uint32_t stride)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    Context& c = ctx->c;
    API_ARG(&c, descriptor < c.heapHost.size(), "descriptor index beyond pt_heap_resize");
    API_ARG(&c, stride == 0 || stride == 2 || stride == 4 || stride == 8, "buffer stride must be 0 (raw), 2 / 4 (typed index buffer) or 8 (structured half4 motion vectors)");
    c.heapHost[descriptor] = HeapEntry{ device_ptr, bytes, stride, kKindBuffer };
    c.heapDirty = true;
    return PT_OK;
}

int pt_heap_set_texture(PtContext* ctx, uint32_t descriptor, const void* device_ptr, uint32_t width, uint32_t height, uint32_t format, uint32_t is_cube)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    Context& c = ctx->c;
    API_ARG(&c, descriptor < c.heapHost.size(), "descriptor index beyond pt_heap_resize");
    API_ARG(&c, device_ptr && width && height, "texture pointer / size is null");
    API_ARG(&c, format <= PT_FORMAT_BC5_UNORM, "unsupported texture format");
    API_ARG(&c, !is_cube || width == height, "cube faces must be square");
    if (format >= PT_FORMAT_BC1_UNORM) {                  // 4x4 blocks, ceil(w / 4) * ceil(h / 4) of them, each read with one aligned vector load
        const bool wide = format == PT_FORMAT_BC3_UNORM || format == PT_FORMAT_BC3_UNORM_SRGB || format == PT_FORMAT_BC5_UNORM;
        API_ARG(&c, !is_cube, "block-compressed cube maps are not supported");
        API_ARG(&c, ((uintptr_t)device_ptr & (wide ? 15u : 7u)) == 0, "block-compressed texture memory must be aligned to its block size (8 bytes for BC1 / BC4, 16 for BC3 / BC5)");
    }
    c.heapHost[descriptor] = HeapEntry{ device_ptr, (uint64_t)width | ((uint64_t)height << 32), format, is_cube ? kKindTextureCube : kKindTexture2D };
    c.heapDirty = true;
    return PT_OK;
}

static int upload_heap(Context& c)
{
    if (!c.srgbLutDev) {                                  // sRGB -> linear table, evaluated in double (arithmetic spec)
        float lut[256];
        for (int i = 0; i < 256; i++) { double v = i / 255.0; lut[i] = (float)(v <= 0.04045 ? v / 12.92 : pow((v + 0.055) / 1.055, 2.4)); }
        API_HIP(&c, upload_once(c.srgbLutDev, lut, sizeof lut));
    }
    if (!c.heapDirty) return PT_OK;
    uint32_t n = (uint32_t)c.heapHost.size();
    c.heapHasTextures = false;
    for (const HeapEntry& e : c.heapHost) if (e.kind != kKindBuffer) c.heapHasTextures = true;
    API_HIP(&c, grow(c.stream, nullptr, want(c.heapDev, n)));
    if (n) API_HIP(&c, hipMemcpyAsync(c.heapDev.data(), c.heapHost.data(), sizeof(HeapEntry) * n, hipMemcpyHostToDevice, c.stream));
    API_HIP(&c, hipStreamSynchronize(c.stream));     // heapHost may change right after
    c.heapDirty = false; c.validated = false;
    return PT_OK;
}

// ---- acceleration structures ----------------------------------------------------------------
static int check_geometries(Context& c, const PtGeometryDesc* geometries, uint32_t geometry_count)
{
    API_ARG(&c, geometries || geometry_count == 0, "geometries is NULL");
    for (uint32_t g = 0; g < geometry_count; g++) {
        // same argument checks as CreateGeometryDesc, Source/RaytracingHelpers.ixx:82-89
        API_ARG(&c, geometries[g].IndexStride == 2 || geometries[g].IndexStride == 4, "Triangle index format must be either uint16 or uint32");
        API_ARG(&c, geometries[g].IndexCount % 3 == 0, "Triangle index count must be divisible by 3");
        API_ARG(&c, geometries[g].IndexCount == 0 || (geometries[g].VertexBuffer && geometries[g].IndexBuffer), "geometry buffer is NULL");
        API_ARG(&c, geometries[g].VertexStride >= 12, "vertex stride must cover a float3 position");
    }
    return PT_OK;
}

static bool any_non_opaque(const PtGeometryDesc* geometries, uint32_t geometry_count)
{
    for (uint32_t g = 0; g < geometry_count; g++) if (!(geometries[g].Flags & PT_GEOMETRY_FLAG_OPAQUE)) return true;
    return false;
}

// the traversal stack holds at most two entries per level of both trees (the rest of a node group and, in the streaming form only, a
// postponed leaf group) plus the three of an instance transition (pt_trace.hpp GroupStack)
static int check_depth(Context& c, uint32_t tlasDepth)
{
    if (2u * (tlasDepth + c.maxBlasDepth) + 4u > (uint32_t)kStackSize)
        return fail(&c, PT_ERROR_INVALID_ARGUMENT, "acceleration structure too deep for the traversal stack (top level " + std::to_string(tlasDepth)
                    + " + bottom level " + std::to_string(c.maxBlasDepth) + " levels)");
    return PT_OK;
}

// the header of the last top-level build arrives asynchronously; look at it as soon as it is there
static int poll_tlas_header(Context& c, bool wait)
{
    if (!c.tlasHeaderPending) return PT_OK;
    if (wait) API_HIP(&c, hipEventSynchronize(c.tlasHeaderEvent.get()));
    else if (hipEventQuery(c.tlasHeaderEvent.get()) != hipSuccess) { (void)hipGetLastError(); return PT_OK; }
    c.tlasHeaderPending = false;
    if (c.tlasHeaderHost.data()->error) { drop_tlas(c); return fail(&c, PT_ERROR_INVALID_ARGUMENT, "top-level build failed: tree deeper than the builder's level limit"); }
    int s = check_depth(c, c.tlasHeaderHost.data()->depth);
    if (s != PT_OK) drop_tlas(c);
    return s;
}

int pt_build_bottom_level(PtContext* ctx, const PtGeometryDesc* geometries, uint32_t geometry_count, uint32_t build_flags, uint64_t* out_blas_id)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    Context& c = ctx->c;
    API_ARG(&c, out_blas_id, "out_blas_id is NULL");
    int s = check_geometries(c, geometries, geometry_count);
    if (s != PT_OK) return s;
    API_HIP(&c, hipSetDevice(c.device));
    Blas b;
    // a static bottom level borrows the context's build buffers (grow-only: the second mesh of a scene allocates nothing but its own
    // nodes and packets); one built for updates keeps buffers of its own
    const bool updatable = (build_flags & PT_BUILD_FLAG_ALLOW_UPDATE) != 0;
    if (!updatable) std::swap(b.tree, c.buildScratch);
    hipError_t e = build_blas_device(geometries, geometry_count, updatable, c.stream, b);
    if (!updatable) std::swap(b.tree, c.buildScratch);
    if (e != hipSuccess) return fail_hip(&c, e, "bottom-level build");
    if (b.buildError || 2u * b.depth + 4u > (uint32_t)kStackSize) return fail(&c, PT_ERROR_INVALID_ARGUMENT, "bottom-level build failed: tree too deep for the traversal stack");
    b.geometryCount = geometry_count;
    b.hasNonOpaque = any_non_opaque(geometries, geometry_count);
    uint64_t id = c.nextBlasId++;
    c.maxBlasDepth = std::max(c.maxBlasDepth, b.depth);
    c.blas[id] = std::move(b);
    *out_blas_id = id;
    return PT_OK;
}

int pt_update_bottom_level(PtContext* ctx, uint64_t blas_id, const PtGeometryDesc* geometries, uint32_t geometry_count, uint32_t build_flags)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    Context& c = ctx->c;
    auto it = c.blas.find(blas_id);
    API_ARG(&c, it != c.blas.end(), "unknown bottom-level id");
    API_ARG(&c, c.viewers.empty(), "other contexts view this context's scene (pt_share_scene): destroy or re-point them before updating a bottom level");
    int s = check_geometries(c, geometries, geometry_count);
    if (s != PT_OK) return s;
    API_HIP(&c, hipSetDevice(c.device));
    Blas& b = it->second;
    uint32_t ntris = 0;
    for (uint32_t g = 0; g < geometry_count; g++) ntris += geometries[g].IndexCount / 3;
    // PERFORM_UPDATE (Source/Scene.ixx:327-341, CommandList::UpdateAccelerationStructures): the skinned vertices moved, the
    // topology did not. A structure built with ALLOW_UPDATE is refitted in place: packets, boxes, quantised nodes; nothing is
    // allocated and nothing waits. The TLAS must be rebuilt afterwards (pt_build_top_level), as the reference does every frame.
    if (b.updatable && ntris == b.triCount && geometry_count == b.geometryCount) {
        hipError_t e = refit_blas_device(geometries, geometry_count, c.stream, b);
        if (e != hipSuccess) return fail_hip(&c, e, "bottom-level update");
        b.hasNonOpaque = any_non_opaque(geometries, geometry_count);   // the refit rewrites the packets' flags from these descriptors
        drop_tlas(c);                                    // instance boxes are stale until the top level is rebuilt
        return PT_OK;
    }
    // not built for updates, or a different triangle count: D3D12 would reject PERFORM_UPDATE; here the structure is rebuilt under its id
    API_HIP(&c, hipStreamSynchronize(c.stream));
    Blas nb;
    const bool updatable = (build_flags & PT_BUILD_FLAG_ALLOW_UPDATE) != 0 || b.updatable;
    if (!updatable) std::swap(nb.tree, c.buildScratch);
    hipError_t e = build_blas_device(geometries, geometry_count, updatable, c.stream, nb);
    if (!updatable) std::swap(nb.tree, c.buildScratch);
    if (e != hipSuccess) return fail_hip(&c, e, "bottom-level update");
    if (nb.buildError || 2u * nb.depth + 4u > (uint32_t)kStackSize) return fail(&c, PT_ERROR_INVALID_ARGUMENT, "bottom-level update failed: tree too deep for the traversal stack");
    // The live top level was accepted over the old tree. A new tree that would take it past the bound is refused here, while the old one
    // is still in place and keeps rendering -- not at the next top-level build, when it is gone. (Without a live top level the update
    // goes through and that build decides.)
    if (c.haveTlas) {
        s = poll_tlas_header(c, true);
        if (s != PT_OK) return s;
    }
    if (c.haveTlas) {
        uint32_t deepest = nb.depth;
        for (auto& kv : c.blas) if (kv.first != blas_id) deepest = std::max(deepest, kv.second.depth);
        const uint32_t tlasDepth = c.tlasHeaderHost.data()->depth;
        if (2u * (tlasDepth + deepest) + 4u > (uint32_t)kStackSize)
            return fail(&c, PT_ERROR_INVALID_ARGUMENT, "bottom-level update failed: the structure would be too deep for the traversal stack (top level " + std::to_string(tlasDepth)
                        + " + bottom level " + std::to_string(deepest) + " levels)");
    }
    nb.geometryCount = geometry_count;
    nb.hasNonOpaque = any_non_opaque(geometries, geometry_count);
    b = std::move(nb);
    c.maxBlasDepth = 0;                                  // over the live bottom levels: the tree that was replaced may have been the deepest
    for (auto& kv : c.blas) c.maxBlasDepth = std::max(c.maxBlasDepth, kv.second.depth);
    drop_tlas(c);                                        // instance records point at the freed arrays
    return PT_OK;
}

int pt_skin_mesh(PtContext* ctx, const void* skeletal_vertices, const float* skeletal_transforms, void* vertices, void* motion_vectors, uint32_t vertex_count)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    Context& c = ctx->c;
    API_ARG(&c, vertex_count == 0 || (skeletal_vertices && skeletal_transforms && vertices && motion_vectors), "a skinning buffer is NULL");
    API_HIP(&c, hipSetDevice(c.device));
    API_HIP(&c, launch_skin(c.stream, skeletal_vertices, skeletal_transforms, vertices, motion_vectors, vertex_count));
    return PT_OK;
}

int pt_release_bottom_level(PtContext* ctx, uint64_t blas_id)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    Context& c = ctx->c;
    auto it = c.blas.find(blas_id);
    API_ARG(&c, it != c.blas.end(), "unknown bottom-level id");
    API_ARG(&c, c.viewers.empty(), "other contexts view this context's scene (pt_share_scene)");
    hipStreamSynchronize(c.stream);
    // the live top level may refer to it (instance records hold its arrays): that top level dies with it, and a render
    // before the next pt_build_top_level answers PT_ERROR_NOT_READY instead of reading freed memory
    for (uint64_t id : c.tlasBlasIds) if (id == blas_id) { drop_tlas(c); break; }
    c.blas.erase(it);
    c.maxBlasDepth = 0;
    for (auto& kv : c.blas) c.maxBlasDepth = std::max(c.maxBlasDepth, kv.second.depth);
    return PT_OK;
}

// ---- the top-level build, in phases: plan (host only) -> allocate -> upload -> launch -> commit. Nothing before the commit changes the
// context's traversal copy, its capacity or where a bottom level lives in it: a build that fails leaves them as they were (drop_tlas has
// put the top level aside, so a render answers PT_ERROR_NOT_READY until the next build succeeds).
//
// Layout of the traversal copy:
//   [ nodes: top level (reserved) | one piece per bottom level ] [ triangle packets per piece ] [ vertex indices per packet ]
//   [ InstanceT x count (API order) ] [ InstanceT x count (top-level leaf order) ] [ entry record x count ]
// Everything that depends on the number of instances sits BEHIND the bottom-level data, and the top level's node reservation only moves
// in steps, so that the pieces keep their places from build to build: a STATIC bottom level lives in the copy only (round 4, VERDICT r3
// item 8). Its first top-level build copies its nodes, packets and indices in and frees the arrays the build left ("adoption"); later
// builds find it in place and copy nothing; when the layout does change (another set of meshes, a top level beyond its reservation) a new
// copy is allocated and the pieces move over from the old one. A bottom level built with ALLOW_UPDATE keeps its own arrays -- the refit
// writes them -- and is copied in every build, as before. Bottom levels that were adopted but are not referenced by this top level ride
// along, so that a later top level can still name them.
namespace {
struct TopLevelPlan {
    struct Piece { uint64_t id; Blas* b; uint32_t nodeBase, triBase; bool referenced; };
    std::vector<Piece> pieces;
    std::vector<uint64_t> pieceIds;
    std::map<uint64_t, uint32_t> pieceOf;
    std::vector<BlasEntry> table;
    uint32_t tlasNodeExact = 0, tlasNodeCap = 0, blobNodes = 0, blobTris = 0;
    uint64_t tris = 0, objectEnd = 0, bindingHash = 1469598103934665603ull, lightHash = 1469598103934665603ull;
    size_t srcBytes = 0, nodeAt = 0, triAt = 0, idxAt = 0, instAt = 0, leafAt = 0, enterAt = 0, total = 0;
    size_t node_at(const Piece& p) const { return nodeAt + sizeof(WideNode) * (size_t)p.nodeBase; }
    size_t tri_at(const Piece& p) const { return triAt + sizeof(TriPacket) * (size_t)p.triBase; }
    size_t idx_at(const Piece& p) const { return idxAt + 16 * (size_t)p.triBase; }
    bool in_place(const Piece& p) const { return p.b->blobNodeAt == node_at(p) && p.b->blobTriAt == tri_at(p) && p.b->blobIdxAt == idx_at(p); }
};
}

// host only: resolve the ids, lay the copy out, write the instance sources into c.tlasUploadHost
// fromDevice (null: none): instances whose transform the device patches in from the posed InstanceData (pt_build_top_level_posed); the
// source's pad word says so to the patch kernel. Nothing else of the plan depends on a transform.
static int plan_top_level(Context& c, const PtInstanceDesc* descs, uint32_t count, const uint8_t* fromDevice, TopLevelPlan& P)
{
    P.tlasNodeExact = wide_node_capacity(count);
    P.tlasNodeCap = P.tlasNodeExact;
    if (count >= 64u) { P.tlasNodeCap = 128u; while (P.tlasNodeCap < P.tlasNodeExact) P.tlasNodeCap <<= 1; }   // (small scenes stay exact: their copy is staged into LDS whole)
    if (c.blobDev && c.tlasNodeReserve >= P.tlasNodeExact && c.tlasNodeReserve <= 2u * P.tlasNodeCap) P.tlasNodeCap = c.tlasNodeReserve;   // keep the reservation of the last build while it fits
    P.blobNodes = P.tlasNodeCap;
    P.lightHash ^= count;
    P.srcBytes = sizeof(InstanceSource) * (size_t)count;
    std::vector<uint8_t>& up = c.tlasUploadHost;
    up.resize(P.srcBytes);
    for (uint32_t i = 0; i < count; i++) {
        auto it = c.blas.find(descs[i].AccelerationStructure);
        API_ARG(&c, it != c.blas.end(), "instance refers to an unknown bottom-level id");
        Blas& b = it->second;
        auto pb = P.pieceOf.find(descs[i].AccelerationStructure);
        if (pb == P.pieceOf.end()) {
            P.pieces.push_back(TopLevelPlan::Piece{ descs[i].AccelerationStructure, &b, P.blobNodes, P.blobTris, true });
            // (pointers of the row are filled in below, once the places are known)
            P.table.push_back(BlasEntry{ nullptr, nullptr, b.rootBounds.data(), b.triCount, b.nodeCount, P.blobNodes, P.blobTris, nullptr, descs[i].InstanceID & 0xFFFFFFu, b.geometryCount });
            P.blobNodes += b.nodeCount; P.blobTris += b.triCount;
            P.pieceIds.push_back(descs[i].AccelerationStructure);
            pb = P.pieceOf.emplace(descs[i].AccelerationStructure, (uint32_t)P.table.size() - 1).first;
        }
        InstanceSource src;
        memcpy(src.transform, descs[i].Transform, sizeof(float) * 12);
        src.instanceID = descs[i].InstanceID & 0xFFFFFFu; src.mask = descs[i].InstanceMask & 0xFFu; src.blasSlot = pb->second; src._pad = fromDevice && fromDevice[i] ? 1u : 0u;
        memcpy(up.data() + sizeof(InstanceSource) * (size_t)i, &src, sizeof src);
        P.tris += b.triCount;
        P.objectEnd = std::max<uint64_t>(P.objectEnd, (uint64_t)src.instanceID + b.geometryCount);
        P.bindingHash = (P.bindingHash ^ src.instanceID) * 1099511628211ull; P.bindingHash = (P.bindingHash ^ descs[i].AccelerationStructure) * 1099511628211ull;
        P.lightHash = (P.lightHash ^ src.instanceID) * 1099511628211ull; P.lightHash = (P.lightHash ^ src.mask) * 1099511628211ull;
        P.lightHash = (P.lightHash ^ descs[i].AccelerationStructure) * 1099511628211ull;
    }
    for (auto& kv : c.blas)                                        // adopted, not referenced: carried along
        if (kv.second.inBlob && !P.pieceOf.count(kv.first)) {
            P.pieces.push_back(TopLevelPlan::Piece{ kv.first, &kv.second, P.blobNodes, P.blobTris, false });
            P.blobNodes += kv.second.nodeCount; P.blobTris += kv.second.triCount;
        }
    const size_t instBytes = (size_t)count * sizeof(InstanceT), nodeBytes = (size_t)P.blobNodes * sizeof(WideNode), triBytes = (size_t)P.blobTris * sizeof(TriPacket);
    const size_t idxBytes = (size_t)P.blobTris * 16;
    P.nodeAt = 0; P.triAt = nodeBytes; P.idxAt = nodeBytes + triBytes; P.instAt = P.idxAt + idxBytes; P.leafAt = P.instAt + instBytes; P.enterAt = P.leafAt + instBytes;
    P.total = P.enterAt + instBytes;
    API_ARG(&c, P.total / 16 < 0xFFFFFFFFull, "scene too large for 32-bit blob addressing");
    return PT_OK;
}

// The one top-level build behind pt_build_top_level (posed == null) and pt_build_top_level_posed.
static int build_top_level(PtContext* ctx, const PtInstanceDesc* descs, uint32_t count, const PtInstanceData* posed, const uint8_t* fromDevice)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    Context& c = ctx->c;
    API_ARG(&c, descs || count == 0, "descs is NULL");
    bool patch = false;
    uint32_t lastPosed = 0;
    for (uint32_t i = 0; fromDevice && i < count; i++) if (fromDevice[i]) { patch = true; lastPosed = i; }
    if (!patch) fromDevice = nullptr;
    API_ARG(&c, !patch || posed, "from_device names instances but device_instances is NULL");
    // the patch kernel reads device_instances[i]: its extent is known only for the array the context has bound
    API_ARG(&c, !patch || (posed == c.instanceData && lastPosed < c.instanceDataCount), "device_instances must be the array bound with pt_set_instance_data and reach every instance from_device names");
    API_ARG(&c, c.viewers.empty(), "other contexts view this context's scene (pt_share_scene): destroy or re-point them before rebuilding");
    API_HIP(&c, hipSetDevice(c.device));
    if (c.sceneOwner) { detach_from_owner(c); drop_tlas(c); }
    int st = poll_tlas_header(c, false);
    if (st != PT_OK) return st;
    TopLevelPlan P;
    st = plan_top_level(c, descs, count, fromDevice, P);
    if (st != PT_OK) return st;

    // ---- allocate: everything is grow-only, so the rebuild of an unchanged scene layout (a dynamic frame) allocates nothing and waits for
    // nothing. A new traversal copy stays local until the commit: its pieces are copied out of the old one first.
    bool moved = false;                                            // an adopted piece is not where the new layout wants it
    for (const auto& p : P.pieces) if (p.b->inBlob && !P.in_place(p)) moved = true;
    const bool newBlob = P.total > c.blobDev.capacity() || moved;
    drop_tlas(c);
    DeviceBuffer<uint8_t> newCopy;                                 // pieces move over from the context's copy into it
    if (newBlob) {
        const hipError_t ea = newCopy.reserve(std::max<size_t>(P.total ? P.total : 16, moved ? c.blobDev.capacity() : 0));
        if (ea != hipSuccess) return fail_hip(&c, ea, "hipMalloc(traversal copy)");
    }
    if (!c.tlasHeaderEvent) API_HIP(&c, create_event(c.tlasHeaderEvent, hipEventDisableTiming));
    if (!c.tlasHeaderHost) API_HIP(&c, c.tlasHeaderHost.reserve(1));
    const uint8_t* oldBlob = c.blobDev.data();
    uint8_t* blob = newBlob ? newCopy.data() : c.blobDev.data();

    // ---- upload, one: instance sources | bottom-level table | copy jobs (first the moves / adoptions of static pieces, which run before
    // anything reads the table; then the per-build copies of updatable pieces and of the top level's nodes, inside the assembly launch)
    std::vector<BlobCopy> preJobs, jobs;
    std::vector<Blas*> adopting;
    for (const auto& p : P.pieces) {
        Blas& b = *p.b;
        uint8_t* dn = blob + P.node_at(p); uint8_t* dt = blob + P.tri_at(p); uint8_t* di = blob + P.idx_at(p);
        const uint64_t n16 = sizeof(WideNode) * (uint64_t)b.nodeCount / 16, t16 = sizeof(TriPacket) * (uint64_t)b.triCount / 16, i16 = b.triCount;
        const void *sn, *st_, *si;
        if (b.updatable) {                                         // own arrays stay the truth: copied in by the assembly launch, read in place by the build's kernels
            jobs.push_back(BlobCopy{ b.nodes.data(), dn, n16 });
            if (b.triCount) { jobs.push_back(BlobCopy{ b.tris.data(), dt, t16 }); jobs.push_back(BlobCopy{ b.idx.data(), di, i16 }); }
            sn = b.nodes.data(); st_ = b.tris.data(); si = b.idx.data();
        } else {
            if (b.inBlob) {
                if (newBlob) {                                     // moves over from the old copy
                    preJobs.push_back(BlobCopy{ oldBlob + b.blobNodeAt, dn, n16 });
                    if (b.triCount) { preJobs.push_back(BlobCopy{ oldBlob + b.blobTriAt, dt, t16 }); preJobs.push_back(BlobCopy{ oldBlob + b.blobIdxAt, di, i16 }); }
                }                                                  // else: in place already
            } else {                                               // first top level that sees it: adopted
                preJobs.push_back(BlobCopy{ b.nodes.data(), dn, n16 });
                if (b.triCount) { preJobs.push_back(BlobCopy{ b.tris.data(), dt, t16 }); preJobs.push_back(BlobCopy{ b.idx.data(), di, i16 }); }
                adopting.push_back(&b);
            }
            sn = dn; st_ = dt; si = di;
        }
        if (p.referenced) { BlasEntry& row = P.table[P.pieceOf[p.id]]; row.nodes = (const WideNode*)sn; row.tris = (const TriPacket*)st_; row.idx = (const uint4*)si; }
    }
    const size_t tableOff = (P.srcBytes + 15) / 16 * 16, tableBytes = sizeof(BlasEntry) * P.table.size();
    const size_t preOff = (tableOff + tableBytes + 15) / 16 * 16, preBytes = sizeof(BlobCopy) * preJobs.size();
    const size_t jobsOff = (preOff + preBytes + 15) / 16 * 16, jobsBytes = sizeof(BlobCopy) * (jobs.size() + 1);   // + the top level's own nodes, below
    std::vector<uint8_t>& up = c.tlasUploadHost;
    up.resize(jobsOff + jobsBytes);
    // everything of the context that this build writes and a frame in flight may read, as one growth with one wait. The upload gets head room:
    // a few more instances next frame do not reallocate. (The build buffers of the top level hold as many items as `instances`: they grow,
    // in build_tlas_prepare, only behind the wait of this growth.)
    const uint32_t instCap = count ? count : 1;
    API_HIP(&c, grow(c.stream, nullptr, want(c.tlas.instances, instCap), want(c.tlas.blasBounds, instCap), want(c.tlas.nodes, wide_node_capacity(instCap)),
                     want(c.tlas.rootBounds, 8), want(c.tlasUploadDev, up.size() > c.tlasUploadDev.capacity() ? up.size() * 2 : 0)));
    hipError_t e = build_tlas_prepare(c.tlas, count);          // the build buffers of the top level (grow-only)
    if (e != hipSuccess) return fail_hip(&c, e, "top-level build");
    jobs.push_back(BlobCopy{ c.tlas.nodes.data(), blob + P.nodeAt, sizeof(WideNode) * (size_t)P.tlasNodeExact / 16 });
    if (tableBytes) memcpy(up.data() + tableOff, P.table.data(), tableBytes);
    if (preBytes) memcpy(up.data() + preOff, preJobs.data(), preBytes);
    memcpy(up.data() + jobsOff, jobs.data(), jobsBytes);
    {
        // staged in pinned host memory, two buffers taken in turn, each guarded by an event recorded behind the copy that read it: the host
        // may be a build ahead of the stream (a dynamic frame never synchronises) without rewriting bytes a copy has yet to read
        Context::UploadStage& sg = c.tlasStage[c.tlasStageNext];
        c.tlasStageNext ^= 1u;
        if (sg.event) API_HIP(&c, hipEventSynchronize(sg.event.get()));   // the copy that last read this buffer has run
        else API_HIP(&c, create_event(sg.event, hipEventDisableTiming));
        if (up.size() > sg.host.capacity()) {                              // (the event, not the stream, guards it: a fresh one, moved in)
            PinnedBuffer<uint8_t> fresh;
            API_HIP(&c, fresh.reserve(up.size() * 2));
            sg.host = std::move(fresh);
        }
        memcpy(sg.host.data(), up.data(), up.size());
        API_HIP(&c, hipMemcpyAsync(c.tlasUploadDev.data(), sg.host.data(), up.size(), hipMemcpyHostToDevice, c.stream));
        API_HIP(&c, hipEventRecord(sg.event.get(), c.stream));
    }
    const uint8_t* upDev = c.tlasUploadDev.data();
    const InstanceSource* dSrc = (const InstanceSource*)upDev;
    const BlasEntry* dTable = (const BlasEntry*)(upDev + tableOff);
    const BlobCopy* dPre = (const BlobCopy*)(upDev + preOff);
    const BlobCopy* dJobs = (const BlobCopy*)(upDev + jobsOff);

    // ---- launch, all in stream order
    if (!preJobs.empty()) e = launch_blob_assembly(nullptr, c.tlas, nullptr, 0, nullptr, nullptr, dPre, (uint32_t)preJobs.size(), nullptr, c.stream);   // static pieces into place first: the table points there
    if (e == hipSuccess && patch) e = launch_patch_instance_sources(c.stream, (InstanceSource*)c.tlasUploadDev.data(), posed, count);
    if (e == hipSuccess) e = launch_instance_records(dSrc, dTable, count, c.tlas.instances.data(), c.tlas.blasBounds.data(), c.tlas.tree.bounds.data(), c.stream);
    if (e == hipSuccess) e = build_tlas_device(c.tlas.instances.data(), c.tlas.blasBounds.data(), count, c.stream, c.tlas);
    if (e == hipSuccess) e = launch_blob_assembly(c.tlas.instances.data(), c.tlas, dTable, count, (InstanceT*)(blob + P.instAt), (InstanceT*)(blob + P.leafAt),
                                                 dJobs, (uint32_t)jobs.size(), (f4v*)(blob + P.enterAt), c.stream);
    if (e == hipSuccess) e = hipMemcpyAsync(c.tlasHeaderHost.data(), c.tlas.tree.header.data(), sizeof(WideHeader), hipMemcpyDeviceToHost, c.stream);
    if (e == hipSuccess) e = hipEventRecord(c.tlasHeaderEvent.get(), c.stream);
    // adoption and moves are load-time events (the first top level of a scene, a change of its meshes): wait for the copies before letting
    // go of what they read. A frame of a dynamic scene over an unchanged set of meshes comes past here with nothing to do.
    if (!adopting.empty() || (newBlob && oldBlob)) {
        const hipError_t es = hipStreamSynchronize(c.stream);
        if (e == hipSuccess) e = es;
    }
    if (e != hipSuccess) {
        if (newCopy) (void)hipStreamSynchronize(c.stream);         // (the launches may still write the new copy, freed on return)
        return fail_hip(&c, e, "top-level build");
    }

    // ---- commit
    if (newBlob) c.blobDev = std::move(newCopy);                   // (frees the old copy)
    for (Blas* b : adopting) { b->nodes.reset(); b->tris.reset(); b->idx.reset(); b->inBlob = true; }
    for (const auto& p : P.pieces) if (p.b->inBlob) { p.b->blobNodeAt = P.node_at(p); p.b->blobTriAt = P.tri_at(p); p.b->blobIdxAt = P.idx_at(p); }
    c.tlasHeaderPending = true;
    c.tlasNodeReserve = P.tlasNodeCap;
    SceneRefs& r = c.scene;
    r.instances = c.tlas.instances.data(); r.instanceCount = count; r.triangleCount = P.tris;
    r.blob.base = (const f4v*)c.blobDev.data();
    r.blob.nodeOff16 = (uint32_t)(P.nodeAt / 16); r.blob.triOff16 = (uint32_t)(P.triAt / 16); r.blob.idxOff16 = (uint32_t)(P.idxAt / 16);
    r.blob.instOff16 = (uint32_t)(P.instAt / 16); r.blob.leafInstOff16 = (uint32_t)(P.leafAt / 16); r.blob.enterOff16 = (uint32_t)(P.enterAt / 16);
    r.blob.instCount = count; r.blob.nodeCount = P.blobNodes; r.blob.triCount = P.blobTris; r.blob.bytes = (uint32_t)P.total;
    r.blasTable = dTable; r.blasTableCount = (uint32_t)P.table.size(); r.instSource = dSrc; r.blasTableMaxTris = 0;
    for (const BlasEntry& te : P.table) r.blasTableMaxTris = std::max(r.blasTableMaxTris, te.triCount);
    r.hasNonOpaque = false;                                         // over the bottom levels this top level refers to (those that only ride along are never entered)
    for (const auto& p : P.pieces) if (p.referenced && p.b->hasNonOpaque) r.hasNonOpaque = true;
    c.tlasBlasIds = P.pieceIds;
    if (P.objectEnd != c.tlasObjectEnd || count != c.tlasValidatedCount || P.bindingHash != c.tlasBindingHash) c.validated = false;     // same instances of the same bottom levels over the same objects: nothing new to check
    c.tlasObjectEnd = P.objectEnd; c.tlasValidatedCount = count; c.tlasBindingHash = P.bindingHash;
    if (P.lightHash != c.tlasLightHash) c.lightListValid = false;
    c.tlasLightHash = P.lightHash;
    // the same instances of the same bottom levels over the same objects (a dynamic frame's rebuild after a refit): the verdict of the
    // shared-geometry check still holds, and with it the frame's normal records (drop_tlas had put them aside with the old top level)
    c.normalsShared = c.validated && c.sharedVerdict;
    c.haveTlas = true;
    return PT_OK;
}

int pt_build_top_level(PtContext* ctx, const PtInstanceDesc* descs, uint32_t count, uint32_t build_flags)
{
    (void)build_flags;
    return build_top_level(ctx, descs, count, nullptr, nullptr);
}

int pt_build_top_level_posed(PtContext* ctx, const PtInstanceDesc* descs, uint32_t count, uint32_t build_flags, const PtInstanceData* device_instances,
                             const uint8_t* from_device)
{
    (void)build_flags;
    return build_top_level(ctx, descs, count, device_instances, from_device);
}

int pt_share_scene(PtContext* ctx, PtContext* source)
{
    if (!ctx || !source || ctx == source) return PT_ERROR_INVALID_ARGUMENT;
    Context& c = ctx->c; Context& s = source->c;
    API_ARG(&c, c.device == s.device, "both contexts must live on the same device");
    API_ARG(&c, c.viewers.empty(), "other contexts view this context's scene");
    API_ARG(&c, !s.sceneOwner, "the source views another context's scene itself: share from the owner");
    API_HIP(&c, hipSetDevice(c.device));
    API_HIP(&c, hipStreamSynchronize(s.stream));
    API_HIP(&c, hipStreamSynchronize(c.stream));
    int st = poll_tlas_header(s, true);
    if (st != PT_OK) return fail(&c, st, s.lastError);
    if (!s.haveTlas) return fail(&c, PT_ERROR_NOT_READY, "the source context has no top-level acceleration structure");
    if (c.sceneOwner) detach_from_owner(c);
    else { API_HIP(&c, materialise_adopted(c)); c.tlas = Tlas(); c.blobDev.reset(); }
    drop_tlas(c);
    c.scene = s.scene;                                                      // views of the owner's
    c.tlasObjectEnd = s.tlasObjectEnd; c.maxBlasDepth = s.maxBlasDepth;
    c.heapHost = s.heapHost; c.heapDirty = true;                            // the descriptor table is copied (each context uploads its own)
    c.objects = s.objects; c.objectCount = s.objectCount; c.instanceData = s.instanceData; c.instanceDataCount = s.instanceDataCount;
    c.sceneOwner = &s; s.viewers.push_back(&c);
    c.tlasHeaderPending = false; c.validated = false;
    c.hasTransmission = c.gbufferTransmission = true;                       // unknown until this context has resolved the object data itself
    c.haveTlas = true;
    return PT_OK;
}

int pt_get_accel_stats(PtContext* ctx, PtAccelStats* out)
{
    if (!ctx || !out) return PT_ERROR_INVALID_ARGUMENT;
    Context& c = ctx->c;
    API_HIP(&c, hipSetDevice(c.device));
    API_HIP(&c, hipStreamSynchronize(c.stream));
    int st = poll_tlas_header(c, true);
    if (st != PT_OK) return st;
    memset(out, 0, sizeof *out);
    out->InstanceCount = c.scene.instanceCount;
    out->BottomLevelCount = (uint32_t)c.blas.size();
    out->TriangleCount = c.scene.triangleCount;
    out->NodeSizeBytes = sizeof(WideNode); out->TriangleSizeBytes = sizeof(TriPacket);
    uint64_t nb = (uint64_t)wide_node_capacity(c.scene.instanceCount) * sizeof(WideNode), tb = 0;
    for (auto& kv : c.blas) { nb += (uint64_t)kv.second.nodeCount * sizeof(WideNode); tb += (uint64_t)kv.second.triCount * sizeof(TriPacket); out->MaxBottomLevelDepth = std::max(out->MaxBottomLevelDepth, kv.second.depth); }
    out->BlobBytes = c.sceneOwner ? 0 : c.scene.blob.bytes;          // a view holds no memory of its own
    out->SharedScene = c.sceneOwner ? 1u : 0u;
    out->NormalRecords = c.normalsShared ? 1u : 0u;
    out->RoundObjectsInLds = round_objects_in_lds(c, c.objectCount, (bool)c.shadeGeomDev);
    out->RoundRecordsInLds = round_records_in_lds(c, c.objectCount, (bool)c.shadeGeomDev);
    if (c.tlasHeaderHost && !c.tlasHeaderPending) out->TopLevelDepth = c.tlasHeaderHost.data()->depth;
    out->NodeBytes = nb; out->TriangleBytes = tb;
    for (auto& kv : c.blas) if (!kv.second.inBlob) out->OwnedBottomLevelBytes += (uint64_t)kv.second.nodeCount * sizeof(WideNode) + (uint64_t)kv.second.triCount * (sizeof(TriPacket) + 16);
    return PT_OK;
}

// ---- per-frame inputs -----------------------------------------------------------------------
int pt_set_camera(PtContext* ctx, const PtCamera* camera)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    API_ARG(&ctx->c, camera, "camera is NULL");
    ctx->c.camera = *camera; ctx->c.haveCamera = true;
    return PT_OK;
}
int pt_set_scene_data(PtContext* ctx, const PtSceneData* scene_data)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    API_ARG(&ctx->c, scene_data, "scene_data is NULL");
    ctx->c.sceneData = *scene_data; ctx->c.haveSceneData = true;
    return PT_OK;
}
int pt_set_object_data(PtContext* ctx, const PtObjectData* device_objects, uint32_t count)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    API_ARG(&ctx->c, device_objects || count == 0, "device_objects is NULL");
    ctx->c.objects = device_objects; ctx->c.objectCount = count;
    return PT_OK;
}
int pt_invalidate_object_data(PtContext* ctx)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    ctx->c.validated = false; ctx->c.normalsShared = false; ctx->c.sharedVerdict = false;   // the next render resolves VertexDesc / MeshDescriptors again (validate_scene)
    ctx->c.hasTransmission = true;                                                            // ... and looks for transmissive materials again: unknown until then
    ctx->c.objectDataGen++;                                                                   // ... and pt_di_render lists the emissive triangles again
    for (pt::Context* v : ctx->c.viewers) { v->validated = false; v->hasTransmission = true; }   // the contexts that view this scene read the same array
    return PT_OK;
}
int pt_set_instance_data(PtContext* ctx, const PtInstanceData* device_instances, uint32_t count)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    ctx->c.instanceData = device_instances; ctx->c.instanceDataCount = count;
    return PT_OK;
}

int pt_set_sharding(PtContext* ctx, const PtSharding* s)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    API_ARG(&ctx->c, s && s->RankCount >= 1 && s->RankIndex < s->RankCount && s->BandHeight >= 1, "invalid sharding");
    ctx->c.sharding = *s;
    return PT_OK;
}

int pt_local_rows(const PtSharding* s, uint32_t frame_height, uint32_t* out_rows)
{
    if (!s || !out_rows || s->RankCount == 0 || s->BandHeight == 0 || s->RankIndex >= s->RankCount) return PT_ERROR_INVALID_ARGUMENT;
    uint32_t rows = 0;
    for (uint32_t b = s->RankIndex; (uint64_t)b * s->BandHeight < frame_height; b += s->RankCount) {
        uint32_t y0 = b * s->BandHeight;
        rows += (frame_height - y0 < s->BandHeight) ? frame_height - y0 : s->BandHeight;
    }
    *out_rows = rows;
    return PT_OK;
}

int pt_deinterleave_bands(PtContext* ctx, void* dst_full, const void* gathered, const uint64_t* rank_offsets_host, uint32_t rank_count,
                          uint32_t band_height, uint32_t width, uint32_t height, uint32_t pixel_bytes)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    Context& c = ctx->c;
    API_ARG(&c, dst_full && gathered && rank_offsets_host && rank_count >= 1 && band_height >= 1, "invalid de-interleave arguments");
    API_ARG(&c, pixel_bytes % 4 == 0, "pixel size must be a multiple of 4 bytes");
    API_HIP(&c, hipSetDevice(c.device));
    API_ARG(&c, rank_count <= 64, "at most 64 ranks");
    hipError_t e = launch_deinterleave(c.stream, dst_full, gathered, rank_offsets_host, rank_count, band_height, width, height, pixel_bytes);
    if (e != hipSuccess) return fail_hip(&c, e, "de-interleave");
    return PT_OK;
}

} // extern "C"

// ---- operators ------------------------------------------------------------------------------
// Scene inputs the kernels will index with: checked once per change of (TLAS, ObjectData binding, heap), never per frame.
// The reference gets these guarantees from D3D12's descriptor heap; here a wrong index would be a wild device read.
static int validate_scene(Context& c)
{
    if (c.validated && c.validatedObjects == c.objects && c.validatedObjectCount == c.objectCount) return PT_OK;
    const uint32_t heapCount = (uint32_t)c.heapHost.size();
    c.hasTransmission = true;                               // unknown until the kernel below has looked (every failure leaves it so)
    if (c.tlasObjectEnd > c.objectCount)
        return fail(&c, PT_ERROR_INVALID_ARGUMENT, "InstanceID + geometry count of an instance reaches ObjectData[" + std::to_string(c.tlasObjectEnd - 1)
                    + "] but only " + std::to_string(c.objectCount) + " objects are bound (pt_set_object_data)");
    if (c.instanceData && c.instanceDataCount < c.scene.instanceCount)
        return fail(&c, PT_ERROR_INVALID_ARGUMENT, "InstanceData holds fewer records than the top level has instances");
    uint32_t sharedMismatch = 0;
    bool transmission = false;                              // no objects: nothing to hit
    if (c.objectCount) {
        // the check's verdict words, and the resolved-geometry tables the same kernel fills (grow-only)
        API_HIP(&c, grow(c.stream, nullptr, want(c.validateDev, 8), want(c.shadeGeomDev, c.objectCount), want(c.shadeTexDev, kTextureSlots * (size_t)c.objectCount)));
        API_HIP(&c, hipMemsetAsync(c.validateDev.data(), 0, sizeof(uint32_t) * 8, c.stream));
        API_HIP(&c, launch_validate_objects(c.stream, c.objects, c.objectCount, c.heapDev.data(), heapCount, c.validateDev.data(), c.shadeGeomDev.data(), c.shadeTexDev.data()));
        // do all instances of a bottom level name the same vertex data? (the frame's normal records are made from the first one's objects)
        if (c.scene.blasTable && c.scene.instSource)
            API_HIP(&c, launch_check_shared_geometry(c.stream, c.scene.instSource, c.scene.blasTable, c.scene.blob.instCount, c.shadeGeomDev.data(), c.validateDev.data()));
        uint32_t r[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
        API_HIP(&c, hipMemcpyAsync(r, c.validateDev.data(), sizeof r, hipMemcpyDeviceToHost, c.stream));
        API_HIP(&c, hipStreamSynchronize(c.stream));
        sharedMismatch = r[4];
        transmission = r[5] != 0u;
        if (r[0]) {
            static const char* what[] = { "", "MeshDescriptors.Vertices", "MeshDescriptors.Indices", "MeshDescriptors.MotionVectors", "TextureMapInfo.Descriptor" };
            return fail(&c, PT_ERROR_INVALID_ARGUMENT, std::string("ObjectData[") + std::to_string(r[1]) + "]." + what[r[0] < 5 ? r[0] : 0] + " = " + std::to_string(r[2])
                        + (r[3] ? " is not the kind of descriptor that member needs" : " is beyond the descriptor heap (" + std::to_string(heapCount) + " descriptors)"));
        }
    }
    c.validated = true; c.validatedObjects = c.objects; c.validatedObjectCount = c.objectCount;
    c.sharedVerdict = c.objectCount != 0 && c.scene.blasTable != nullptr && sharedMismatch == 0;
    c.normalsShared = c.sharedVerdict;
    c.hasTransmission = transmission;
    return PT_OK;
}

int pt::make_views(Context& c, uint32_t width, uint32_t height, SceneView& sv, FrameView& fv, bool needFrameInputs)
{
    // A top level whose build has not reported back yet is never rendered: its depth / error word decides whether the traversal stack can
    // walk it at all. One wait per BUILD (for the build's own kernels, ~0.3 ms of stream work that the frame needs anyway), none per frame
    // of a static scene; the rest of the frame is enqueued without waiting.
    int s = poll_tlas_header(c, true);
    if (s != PT_OK) return s;
    if (!c.haveTlas) return fail(&c, PT_ERROR_NOT_READY, "no top-level acceleration structure: call pt_build_top_level first");
    if (needFrameInputs && (!c.haveCamera || !c.haveSceneData)) return fail(&c, PT_ERROR_NOT_READY, "camera / scene data not set");
    if (!c.objects && c.scene.instanceCount) return fail(&c, PT_ERROR_NOT_READY, "object data not set");
    s = upload_heap(c);
    if (s != PT_OK) return s;
    s = validate_scene(c);
    if (s != PT_OK) return s;
    if (needFrameInputs && c.sceneData.EnvironmentLightTextureDescriptor != ~0u) {
        const uint32_t d = c.sceneData.EnvironmentLightTextureDescriptor;
        API_ARG(&c, d < c.heapHost.size(), "SceneData.EnvironmentLightTextureDescriptor is beyond the descriptor heap");
        API_ARG(&c, c.heapHost[d].kind == (c.sceneData.IsEnvironmentLightTextureCubeMap ? kKindTextureCube : kKindTexture2D),
                "SceneData.EnvironmentLightTextureDescriptor is not the kind of texture IsEnvironmentLightTextureCubeMap says");
    }
    sv.accel.instances = c.scene.instances; sv.accel.instanceCount = c.scene.instanceCount;
    sv.objects = c.objects; sv.objectCount = c.objectCount; sv.shadeGeom = c.shadeGeomDev.data(); sv.shadeTex = c.shadeTexDev.data();
    sv.instanceData = c.instanceData;
    sv.heap = c.heapDev.data(); sv.heapCount = (uint32_t)c.heapHost.size();
    sv.srgbLut = c.srgbLutDev.data();
    fv.width = width; fv.height = height;
    fv.rankIndex = c.sharding.RankIndex; fv.rankCount = c.sharding.RankCount; fv.bandHeight = c.sharding.BandHeight;
    pt_local_rows(&c.sharding, height, &fv.localRows);
    return PT_OK;
}

// (the SHARC entry point has narrowed Denoiser to None / DLSS-RR before it comes here: the two Denoiser checks cannot fire for it)
int pt::check_raytrace_args(Context& c, const PtTextures* tx)
{
    API_ARG(&c, c.settings.Denoiser <= PT_DENOISER_NRD_RELAX, "unknown Denoiser value");
    const bool empty = !rank_holds_pixels(c, c.settings.RenderSize[0], c.settings.RenderSize[1]);   // nothing to bind: the pass launches nothing
    API_ARG(&c, empty || !c.settings.IsDIEnabled || (tx->Diffuse && tx->Specular), "IsDIEnabled reads the direct lighting from Textures.Diffuse / Textures.Specular (pt_di_render): not bound");
    API_ARG(&c, empty || !(c.settings.Denoiser >= PT_DENOISER_NRD_REBLUR) || (tx->Diffuse && tx->Specular), "NRD modes write Textures.Diffuse / Textures.Specular: not bound");
    API_ARG(&c, c.settings.SamplesPerPixel < 65536 && c.settings.Bounces < 32768, "SamplesPerPixel / Bounces out of range");
    API_ARG(&c, empty || (tx->Position && tx->FlatNormal && tx->GeometricNormal && tx->BaseColorMetalness && tx->NormalRoughness && tx->IOR
                          && tx->Transmission && tx->Radiance), "a G-buffer texture the path tracer reads is not bound (Raytracing::Textures)");
    return PT_OK;
}

// A rank whose bands all lie below the frame holds no rows (a 5-row frame in bands of 16 over three ranks leaves two of them empty). Its textures
// are allocations of zero bytes, which may well be NULL: the render operators ask for no binding there and launch nothing.
bool pt::rank_holds_pixels(const Context& c, uint32_t width, uint32_t height)
{
    uint32_t rows = 0;
    pt_local_rows(&c.sharding, height, &rows);
    return width != 0u && rows != 0u;
}

extern "C" {

int pt_gbuffer_render(PtContext* ctx, const PtGBufferConstants* constants, const PtTextures* textures)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    Context& c = ctx->c;
    API_ARG(&c, constants && textures, "constants / textures is NULL");
    API_HIP(&c, hipSetDevice(c.device));
    SceneView sv; FrameView fv; memset(&sv, 0, sizeof sv); memset(&fv, 0, sizeof fv);
    int s = make_views(c, constants->RenderSize[0], constants->RenderSize[1], sv, fv);
    if (s != PT_OK) return s;
    API_HIP(&c, launch_gbuffer(c, sv, fv, constants->Flags, *textures));
    return PT_OK;
}

int pt_raytrace_set_constants(PtContext* ctx, const PtGraphicsSettings* settings)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    API_ARG(&ctx->c, settings, "settings is NULL");
    ctx->c.settings = *settings; ctx->c.haveSettings = true;
    return PT_OK;
}

int pt_raytrace_render(PtContext* ctx, const PtTextures* tx)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    Context& c = ctx->c;
    API_ARG(&c, tx, "textures is NULL");
    if (!c.haveSettings) return fail(&c, PT_ERROR_NOT_READY, "call pt_raytrace_set_constants first");
    int s = check_raytrace_args(c, tx);
    if (s != PT_OK) return s;
    API_HIP(&c, hipSetDevice(c.device));
    SceneView sv; FrameView fv; memset(&sv, 0, sizeof sv); memset(&fv, 0, sizeof fv);
    s = make_views(c, c.settings.RenderSize[0], c.settings.RenderSize[1], sv, fv);
    if (s != PT_OK) return s;
    if (c.settings.Bounces == 0) return PT_OK;          // reference: the pass is not dispatched, Source/App.cpp:1277-1279
    API_HIP(&c, launch_raytrace(c, sv, fv, *tx, false));
    return PT_OK;
}

int pt_trace_visibility(PtContext* ctx, const PtRayDesc* device_rays, uint32_t count, float* device_visibility)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    Context& c = ctx->c;
    API_ARG(&c, count == 0 || (device_rays && device_visibility), "ray / visibility buffer is NULL");
    API_HIP(&c, hipSetDevice(c.device));
    SceneView sv; FrameView fv; memset(&sv, 0, sizeof sv); memset(&fv, 0, sizeof fv);
    int s = make_views(c, 1, 1, sv, fv, false);                    // only the scene half of the views is needed
    if (s != PT_OK) return s;
    API_HIP(&c, launch_visibility(c, sv, device_rays, count, device_visibility));
    return PT_OK;
}

int pt_bsdf_evaluate(PtContext* ctx, const PtBsdfQuery* device_queries, uint32_t count, PtBsdfResult* device_results)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    Context& c = ctx->c;
    API_ARG(&c, count == 0 || (device_queries && device_results), "query / result buffer is NULL");
    API_HIP(&c, hipSetDevice(c.device));
    API_HIP(&c, launch_bsdf_evaluate(c.stream, (const float*)device_queries, count, (float*)device_results));
    return PT_OK;
}

int pt_bsdf_sample(PtContext* ctx, const PtBsdfSampleQuery* device_queries, uint32_t count, PtBsdfSampleResult* device_results)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    Context& c = ctx->c;
    API_ARG(&c, count == 0 || (device_queries && device_results), "query / result buffer is NULL");
    API_HIP(&c, hipSetDevice(c.device));
    API_HIP(&c, launch_bsdf_sample(c.stream, (const float*)device_queries, count, (float*)device_results, !(c.debugFlags & PT_DEBUG_GENERIC_SCENE)));
    return PT_OK;
}

// ---- measurement ----------------------------------------------------------------------------
int pt_reset_counters(PtContext* ctx)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    API_HIP(&ctx->c, hipSetDevice(ctx->c.device));
    API_HIP(&ctx->c, hipMemsetAsync(ctx->c.counters.data(), 0, sizeof(DeviceCounters), ctx->c.stream));
    return PT_OK;
}

int pt_get_counters(PtContext* ctx, PtCounters* out)
{
    if (!ctx || !out) return PT_ERROR_INVALID_ARGUMENT;
    Context& c = ctx->c;
    API_HIP(&c, hipSetDevice(c.device));
    DeviceCounters d;
    API_HIP(&c, hipMemcpyAsync(&d, c.counters.data(), sizeof d, hipMemcpyDeviceToHost, c.stream));
    API_HIP(&c, hipStreamSynchronize(c.stream));
    memset(out, 0, sizeof *out);
    out->PrimaryRays = d.primaryRays; out->SecondaryRays = d.secondaryRays;
    out->NodesVisited = d.nodesVisited; out->TrianglesTested = d.trianglesTested;
    out->WavefrontIterations = c.lastIterations;
    out->BvhMismatches = d.mismatchCount;
    out->StackOverflows = d.stackOverflows;
    out->MaxNodesPerRay = d.maxNodesPerRay;
    return PT_OK;
}

int pt_debug_read_mismatch(PtContext* ctx, float* out16)
{
    if (!ctx || !out16) return PT_ERROR_INVALID_ARGUMENT;
    Context& c = ctx->c;
    API_HIP(&c, hipSetDevice(c.device));
    DeviceCounters d;
    API_HIP(&c, hipMemcpyAsync(&d, c.counters.data(), sizeof d, hipMemcpyDeviceToHost, c.stream));
    API_HIP(&c, hipStreamSynchronize(c.stream));
    memcpy(out16, d.mismatchRay, sizeof(float) * 16);
    return PT_OK;
}

int pt_debug_download_blob(PtContext* ctx, void* host_dst, uint64_t capacity_bytes, PtBlobLayout* out_layout)
{
    if (!ctx || !out_layout) return PT_ERROR_INVALID_ARGUMENT;
    Context& c = ctx->c;
    API_HIP(&c, hipSetDevice(c.device));
    API_HIP(&c, hipStreamSynchronize(c.stream));
    int st = poll_tlas_header(c, true);
    if (st != PT_OK) return st;
    if (!c.haveTlas) return fail(&c, PT_ERROR_NOT_READY, "no top-level acceleration structure");
    const BlobView& b = c.scene.blob;
    *out_layout = PtBlobLayout{ b.instOff16, b.nodeOff16, b.triOff16, b.leafInstOff16, b.instCount, b.nodeCount, b.triCount, b.bytes };
    if (host_dst) {
        API_ARG(&c, capacity_bytes >= b.bytes, "host buffer smaller than the blob");
        API_HIP(&c, hipMemcpy(host_dst, b.base, b.bytes, hipMemcpyDeviceToHost));
    }
    return PT_OK;
}

int pt_debug_trace_ray(PtContext* ctx, const PtRayDesc* host_ray, uint32_t* host_log, uint32_t log_words)
{
    if (!ctx || !host_ray || !host_log) return PT_ERROR_INVALID_ARGUMENT;
    Context& c = ctx->c;
    API_HIP(&c, hipSetDevice(c.device));
    SceneView sv; FrameView fv; memset(&sv, 0, sizeof sv); memset(&fv, 0, sizeof fv);
    int s = make_views(c, 1, 1, sv, fv, false);
    if (s != PT_OK) return s;
    DeviceBuffer<uint32_t> dev;
    API_HIP(&c, dev.reserve(log_words ? log_words : 4));
    hipError_t e = hipMemsetAsync(dev.data(), 0, sizeof(uint32_t) * log_words, c.stream);
    if (e == hipSuccess) e = launch_debug_trace(c, sv, (const float*)host_ray, dev.data(), log_words);
    if (e == hipSuccess) e = hipMemcpyAsync(host_log, dev.data(), sizeof(uint32_t) * log_words, hipMemcpyDeviceToHost, c.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c.stream);
    if (e != hipSuccess) return fail_hip(&c, e, "debug trace");
    return PT_OK;
}

int pt_debug_trace_closest(PtContext* ctx, const PtRayDesc* device_rays, uint32_t count, PtClosestHit* device_hits)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    Context& c = ctx->c;
    API_ARG(&c, count == 0 || (device_rays && device_hits), "ray / hit buffer is NULL");
    API_HIP(&c, hipSetDevice(c.device));
    SceneView sv; FrameView fv; memset(&sv, 0, sizeof sv); memset(&fv, 0, sizeof fv);
    int s = make_views(c, 1, 1, sv, fv, false);                    // only the scene half of the views is needed
    if (s != PT_OK) return s;
    API_HIP(&c, launch_debug_closest(c, sv, device_rays, count, device_hits));
    return PT_OK;
}

int pt_set_debug_flags(PtContext* ctx, uint32_t flags)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    ctx->c.debugFlags = flags;
    return PT_OK;
}

int pt_enable_kernel_timing(PtContext* ctx, int enable)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    ctx->c.timing = enable != 0;
    ctx->c.nExtend = ctx->c.nShade = ctx->c.nRound = 0;          // accumulation restarts
    return PT_OK;
}

int pt_get_kernel_timing(PtContext* ctx, float* extend_ms, float* shade_ms, uint32_t* extend_launches, uint32_t* shade_launches)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    Context& c = ctx->c;
    API_HIP(&c, hipSetDevice(c.device));
    API_HIP(&c, hipStreamSynchronize(c.stream));
    float te = 0.0f, ts = 0.0f;
    if (c.timing) {
        for (uint32_t k = 0; k < c.nExtend && 2 * k + 1 < c.evExtend.size(); k++) { float ms = 0; hipEventElapsedTime(&ms, c.evExtend[2 * k].get(), c.evExtend[2 * k + 1].get()); te += ms; }
        for (uint32_t k = 0; k < c.nShade && 2 * k + 1 < c.evShade.size(); k++) { float ms = 0; hipEventElapsedTime(&ms, c.evShade[2 * k].get(), c.evShade[2 * k + 1].get()); ts += ms; }
    }
    if (extend_ms) *extend_ms = te;
    if (shade_ms) *shade_ms = ts;
    if (extend_launches) *extend_launches = c.nExtend;
    if (shade_launches) *shade_launches = c.nShade;
    return PT_OK;
}

int pt_get_round_timing(PtContext* ctx, float* round_ms, uint32_t* round_launches)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    Context& c = ctx->c;
    API_HIP(&c, hipSetDevice(c.device));
    API_HIP(&c, hipStreamSynchronize(c.stream));
    float t = 0.0f;
    if (c.timing)
        for (uint32_t k = 0; k < c.nRound && 2 * k + 1 < c.evRound.size(); k++) { float ms = 0; hipEventElapsedTime(&ms, c.evRound[2 * k].get(), c.evRound[2 * k + 1].get()); t += ms; }
    if (round_ms) *round_ms = t;
    if (round_launches) *round_launches = c.nRound;
    return PT_OK;
}

} // extern "C"
