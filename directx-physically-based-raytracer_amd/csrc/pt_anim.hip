// pt_anim.hip -- animation playback on the device (gfx950): the per-frame half of Source/Animation.ixx and Scene::Refresh.
//
//   k_anim_pose              <- KeyframeCollection::Interpolate (Animation.ixx:45-75), Animation::ComputeTransforms (:119-162) and the
//                               instance transforms of Scene::Refresh (Scene.ixx:195-231), for every state of pt_anim_evaluate in ONE launch:
//                               one workgroup of 64 lanes per animated object. Lanes take nodes; the hierarchy runs level by level (the rig
//                               keeps its nodes ordered by depth), a workgroup barrier between levels; then the skins' inverses, then joints
//                               and instance bindings side by side.
//   k_patch_instance_sources <- pt_build_top_level_posed: the transforms of the uploaded instance sources, from the posed InstanceData
// These kernels are latency-bound (a few hundred matrices): what counts is the number of launches, one per call, whatever the object count.
// DESIGN.md section 1, "Animation", is the arithmetic spec: fp32, every product and sum rounded on its own (the file is compiled with
// contraction off), key times compared and the key fraction formed in fp64.
#include "pt_internal.hpp"

#include <cmath>
#include <cstring>

namespace pt {

constexpr int kAnimLanes = 64;
constexpr uint32_t kNoNode = PT_ANIM_NO_NODE;

// ---- arithmetic -------------------------------------------------------------------------------------------------------------------------
// C = A . B, row-vector convention, each entry ((a0 b0 + a1 b1) + a2 b2) + a3 b3
__device__ __forceinline__ void anim_mul(const float* A, const float* B, float* C)
{
    #pragma unroll
    for (int i = 0; i < 4; i++) {
        #pragma unroll
        for (int j = 0; j < 4; j++)
            C[4 * i + j] = ((A[4 * i] * B[j] + A[4 * i + 1] * B[4 + j]) + A[4 * i + 2] * B[8 + j]) + A[4 * i + 3] * B[12 + j];
    }
}

// general 4x4 inverse by cofactors (2x2 sub-determinants of the upper and the lower row pair)
__device__ __forceinline__ void anim_inverse(const float* m, float* o)
{
    const float s0 = m[0] * m[5] - m[4] * m[1], s1 = m[0] * m[6] - m[4] * m[2], s2 = m[0] * m[7] - m[4] * m[3];
    const float s3 = m[1] * m[6] - m[5] * m[2], s4 = m[1] * m[7] - m[5] * m[3], s5 = m[2] * m[7] - m[6] * m[3];
    const float c5 = m[10] * m[15] - m[14] * m[11], c4 = m[9] * m[15] - m[13] * m[11], c3 = m[9] * m[14] - m[13] * m[10];
    const float c2 = m[8] * m[15] - m[12] * m[11], c1 = m[8] * m[14] - m[12] * m[10], c0 = m[8] * m[13] - m[12] * m[9];
    const float det = ((((s0 * c5 - s1 * c4) + s2 * c3) + s3 * c2) - s4 * c1) + s5 * c0;
    const float r = 1.0f / det;
    o[0]  = (( m[5] * c5 - m[6] * c4) + m[7] * c3) * r;
    o[1]  = ((-m[1] * c5 + m[2] * c4) - m[3] * c3) * r;
    o[2]  = (( m[13] * s5 - m[14] * s4) + m[15] * s3) * r;
    o[3]  = ((-m[9] * s5 + m[10] * s4) - m[11] * s3) * r;
    o[4]  = ((-m[4] * c5 + m[6] * c2) - m[7] * c1) * r;
    o[5]  = (( m[0] * c5 - m[2] * c2) + m[3] * c1) * r;
    o[6]  = ((-m[12] * s5 + m[14] * s2) - m[15] * s1) * r;
    o[7]  = (( m[8] * s5 - m[10] * s2) + m[11] * s1) * r;
    o[8]  = (( m[4] * c4 - m[5] * c2) + m[7] * c0) * r;
    o[9]  = ((-m[0] * c4 + m[1] * c2) - m[3] * c0) * r;
    o[10] = (( m[12] * s4 - m[13] * s2) + m[15] * s0) * r;
    o[11] = ((-m[8] * s4 + m[9] * s2) - m[11] * s0) * r;
    o[12] = ((-m[4] * c3 + m[5] * c1) - m[6] * c0) * r;
    o[13] = (( m[0] * c3 - m[1] * c1) + m[2] * c0) * r;
    o[14] = ((-m[12] * s3 + m[13] * s1) - m[14] * s0) * r;
    o[15] = (( m[8] * s3 - m[9] * s1) + m[10] * s0) * r;
}

// XMQuaternionSlerp's structure; not renormalised. dbg (8 floats, may be null): c, x, s, w, a0, a1, sin a0, sin a1
__device__ __forceinline__ float4 anim_slerp(float4 q0, float4 q1, float t, float* dbg)
{
    float c = ((q0.x * q1.x + q0.y * q1.y) + q0.z * q1.z) + q0.w * q1.w;
    if (c < 0.0f) { c = -c; q1 = make_float4(-q1.x, -q1.y, -q1.z, -q1.w); }
    float w0, w1;
    if (dbg) { dbg[0] = c; for (int k = 1; k < 8; k++) dbg[k] = 0.0f; }
    if (c > 1.0f - 1e-5f) { w0 = 1.0f - t; w1 = t; }
    else {
        const float x = 1.0f - c * c;
        const float s = sqrtf(x);
        const float w = atan2f(s, c);
        const float a0 = (1.0f - t) * w, a1 = t * w;
        const float n0 = sinf(a0), n1 = sinf(a1);
        w0 = n0 / s; w1 = n1 / s;
        if (dbg) { dbg[1] = x; dbg[2] = s; dbg[3] = w; dbg[4] = a0; dbg[5] = a1; dbg[6] = n0; dbg[7] = n1; }
    }
    return make_float4(w0 * q0.x + w1 * q1.x, w0 * q0.y + w1 * q1.y, w0 * q0.z + w1 * q1.z, w0 * q0.w + w1 * q1.w);
}

// KeyframeCollection::Interpolate without the matrix: the value of a channel at `time`. Before the first key: the first value; at or after
// the last: the last; else keys i = upper_bound - 1 and i + 1 with t = float((time - t0) / (t1 - t0)) in fp64.
template <bool ROTATION>
__device__ __forceinline__ float4 anim_channel(const float* __restrict__ times, const float4* __restrict__ values, uint2 ch, double time)
{
    const float* kt = times + ch.x; const float4* kv = values + ch.x;
    if (time < (double)kt[0]) return kv[0];
    uint32_t lo = 0, hi = ch.y;                      // upper_bound: the first key whose time is > time
    while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if ((double)kt[mid] <= time) lo = mid + 1; else hi = mid; }
    if (lo == ch.y) return kv[ch.y - 1];
    const uint32_t i = lo - 1;
    const double t0 = (double)kt[i], t1 = (double)kt[i + 1];
    const float t = (float)((time - t0) / (t1 - t0));
    const float4 a = kv[i], b = kv[i + 1];
    if (ROTATION) return anim_slerp(a, b, t, nullptr);
    return make_float4(a.x + t * (b.x - a.x), a.y + t * (b.y - a.y), a.z + t * (b.z - a.z), 0.0f);
}

// local = S . R . T: the rows of XMMatrixRotationQuaternion(q) scaled, the translation in the last row (the products with the zeros and
// ones of S and T are exact: these are the bits of the two full products)
__device__ __forceinline__ void anim_local(float4 tr, float4 q, float4 sc, float* L)
{
    const float xx = q.x * q.x, yy = q.y * q.y, zz = q.z * q.z;
    const float xy = q.x * q.y, xz = q.x * q.z, yz = q.y * q.z, xw = q.x * q.w, yw = q.y * q.w, zw = q.z * q.w;
    const float r00 = 1.0f - 2.0f * (yy + zz), r01 = 2.0f * (xy + zw), r02 = 2.0f * (xz - yw);
    const float r10 = 2.0f * (xy - zw), r11 = 1.0f - 2.0f * (xx + zz), r12 = 2.0f * (yz + xw);
    const float r20 = 2.0f * (xz + yw), r21 = 2.0f * (yz - xw), r22 = 1.0f - 2.0f * (xx + yy);
    L[0] = sc.x * r00; L[1] = sc.x * r01; L[2] = sc.x * r02; L[3] = 0.0f;
    L[4] = sc.y * r10; L[5] = sc.y * r11; L[6] = sc.y * r12; L[7] = 0.0f;
    L[8] = sc.z * r20; L[9] = sc.z * r21; L[10] = sc.z * r22; L[11] = 0.0f;
    L[12] = tr.x; L[13] = tr.y; L[14] = tr.z; L[15] = 1.0f;
}

// XMStoreFloat3x4: the transpose's first three rows (rows of the column-vector affine [R|t])
__device__ __forceinline__ void anim_store3x4(const float* M, float* out)
{
    #pragma unroll
    for (int r = 0; r < 3; r++) {
        #pragma unroll
        for (int k = 0; k < 4; k++) out[4 * r + k] = M[4 * k + r];
    }
}

__global__ __launch_bounds__(kAnimLanes) void k_anim_pose(const AnimStateDev* __restrict__ states, PtInstanceData* instances)
{
    const AnimStateDev st = states[blockIdx.x];
    const AnimObjectView* o = st.object;
    const AnimRigView g = o->rig;
    float* G = o->globals;
    const uint32_t lane = threadIdx.x;

    // locals, into the node's slot of the globals
    const uint2* ch = g.channels + (size_t)st.clip * g.nodeCount * 3u;
    for (uint32_t n = lane; n < g.nodeCount; n += kAnimLanes) {
        const float* rest = g.rest + 10u * n;
        float4 tr = make_float4(rest[0], rest[1], rest[2], 0.0f), q = make_float4(rest[3], rest[4], rest[5], rest[6]), sc = make_float4(rest[7], rest[8], rest[9], 0.0f);
        const uint2 ct = ch[3u * n], cr = ch[3u * n + 1u], cs = ch[3u * n + 2u];
        if (ct.y) tr = anim_channel<false>(g.keyTimes, g.keyValues, ct, st.time);
        if (cr.y) q = anim_channel<true>(g.keyTimes, g.keyValues, cr, st.time);
        if (cs.y) sc = anim_channel<false>(g.keyTimes, g.keyValues, cs, st.time);
        float L[16];
        anim_local(tr, q, sc, L);
        #pragma unroll
        for (int k = 0; k < 16; k++) G[16u * n + k] = L[k];
    }
    __syncthreads();
    // global = local . Global(parent), one level of the forest at a time (level 0, the roots: the local transform as it is)
    for (uint32_t l = 1; l < g.levelCount; l++) {
        const uint32_t end = g.levelStart[l + 1];
        for (uint32_t k = g.levelStart[l] + lane; k < end; k += kAnimLanes) {
            const uint32_t n = g.levelNodes[k];
            float L[16], P[16], M[16];
            #pragma unroll
            for (int e = 0; e < 16; e++) { L[e] = G[16u * n + e]; P[e] = G[16u * (uint32_t)g.parents[n] + e]; }
            anim_mul(L, P, M);
            #pragma unroll
            for (int e = 0; e < 16; e++) G[16u * n + e] = M[e];
        }
        __syncthreads();
    }
    // Global(meshNode)^-1 per skin
    for (uint32_t s = lane; s < o->skinCount; s += kAnimLanes) {
        const uint32_t mn = o->skinMeshNodes[s];
        if (mn == kNoNode) continue;
        float M[16], I[16];
        #pragma unroll
        for (int e = 0; e < 16; e++) M[e] = G[16u * mn + e];
        anim_inverse(M, I);
        #pragma unroll
        for (int e = 0; e < 16; e++) o->skinInverse[16u * s + e] = I[e];
    }
    __syncthreads();
    // skeletal transforms: (InverseBind . Global(joint)) . Global(meshNode)^-1. A joint or a mesh node without a rig node keeps its matrix.
    for (uint32_t j = lane; j < o->jointCount; j += kAnimLanes) {
        const uint32_t s = o->jointSkin[j], jn = o->jointNodes[j];
        if (jn == kNoNode || o->skinMeshNodes[s] == kNoNode) continue;
        float A[16], B[16], M[16];
        #pragma unroll
        for (int e = 0; e < 16; e++) { A[e] = o->inverseBinds[16u * j + e]; B[e] = G[16u * jn + e]; }
        anim_mul(A, B, M);
        #pragma unroll
        for (int e = 0; e < 16; e++) B[e] = o->skinInverse[16u * s + e];
        anim_mul(M, B, A);
        anim_store3x4(A, o->skeletal + 12u * j);
    }
    // instance transforms: (Global(meshNode) . Scale(1, 1, -1)) . RenderObject.Transform
    if (instances) {
        for (uint32_t b = lane; b < o->bindingCount; b += kAnimLanes) {
            const uint32_t node = o->bindingNodes[b];
            const float* src = node == kNoNode ? o->bindingGlobals + 16u * b : G + 16u * node;
            float A[16], T[16], M[16], now[12];
            #pragma unroll
            for (int e = 0; e < 16; e++) { A[e] = (e & 3) == 2 ? -src[e] : src[e]; T[e] = o->transform[e]; }
            anim_mul(A, T, M);
            anim_store3x4(M, now);
            PtInstanceData* id = instances + o->bindingInstances[b];
            #pragma unroll
            for (int e = 0; e < 12; e++) {
                id->PreviousObjectToWorld[e] = st.first ? now[e] : id->ObjectToWorld[e];
                id->ObjectToWorld[e] = now[e];
            }
        }
    }
}

__global__ void k_patch_instance_sources(InstanceSource* __restrict__ src, const PtInstanceData* __restrict__ instances, uint32_t n)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !src[i]._pad) return;
    #pragma unroll
    for (int e = 0; e < 12; e++) src[i].transform[e] = instances[i].ObjectToWorld[e];
}

hipError_t launch_patch_instance_sources(hipStream_t stream, InstanceSource* src, const PtInstanceData* instances, uint32_t n)
{
    if (!n) return hipSuccess;
    k_patch_instance_sources<<<(n + 255u) / 256u, 256, 0, stream>>>(src, instances, n);
    return hipGetLastError();
}

__global__ void k_anim_debug_slerp(const float4* __restrict__ q0, const float4* __restrict__ q1, const float* __restrict__ t, uint32_t n, float* __restrict__ out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float dbg[8];
    const float4 q = anim_slerp(q0[i], q1[i], t[i], dbg);
    float* o = out + 12u * i;
    o[0] = q.x; o[1] = q.y; o[2] = q.z; o[3] = q.w;
    for (int k = 0; k < 8; k++) o[4 + k] = dbg[k];
}

// ---- host -------------------------------------------------------------------------------------------------------------------------------
// sections of one device buffer, 16-byte aligned, laid out on the host and uploaded with one copy
struct Packer {
    std::vector<uint8_t> bytes;
    size_t add(const void* p, size_t n) { const size_t at = (bytes.size() + 15) / 16 * 16; bytes.resize(at + n); if (n && p) memcpy(bytes.data() + at, p, n); return at; }
};

static bool all_finite(const float* p, size_t n) { for (size_t i = 0; i < n; i++) if (!std::isfinite(p[i])) return false; return true; }

} // namespace pt

using namespace pt;

extern "C" {

int pt_anim_create_rig(PtContext* ctx, uint32_t node_count, const int32_t* parents, const float* rest_trs, uint32_t clip_count, const double* durations,
                       const uint32_t* channels, const float* key_times, const float* key_values, uint32_t key_count, uint64_t* out_rig)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    Context& c = ctx->c;
    API_ARG(&c, out_rig, "out_rig is NULL");
    API_ARG(&c, node_count >= 1 && node_count <= (1u << 20) && parents && rest_trs, "a rig needs 1 .. 2^20 nodes with parents and rest transforms");
    API_ARG(&c, clip_count >= 1 && clip_count <= 4096u && durations && channels, "a rig needs 1 .. 4096 clips with durations and channels");
    API_ARG(&c, key_count == 0 || (key_times && key_values), "key_times / key_values is NULL");
    std::vector<uint32_t> depth(node_count), levelStart;
    uint32_t levels = 0;
    for (uint32_t n = 0; n < node_count; n++) {
        API_ARG(&c, parents[n] >= -1 && (parents[n] < 0 || (uint32_t)parents[n] < n), "a node's Parent must be -1 or below the node's own index");
        depth[n] = parents[n] < 0 ? 0 : depth[parents[n]] + 1;
        levels = std::max(levels, depth[n] + 1);
    }
    API_ARG(&c, all_finite(rest_trs, 10 * (size_t)node_count), "a rest Translation / Rotation / Scale is not finite");
    API_ARG(&c, all_finite(key_times, key_count), "a key time is not finite");
    API_ARG(&c, all_finite(key_values, 4 * (size_t)key_count), "a key value is not finite");
    for (uint32_t k = 0; k < clip_count; k++) API_ARG(&c, std::isfinite(durations[k]) && durations[k] >= 0.0, "a clip's Duration is negative or not finite");
    const size_t nch = (size_t)clip_count * node_count * 3;
    for (size_t k = 0; k < nch; k++) {
        const uint32_t first = channels[2 * k], n = channels[2 * k + 1];
        if (!n) continue;
        API_ARG(&c, first <= key_count && n <= key_count - first, "a channel runs beyond the keys");
        for (uint32_t i = 1; i < n; i++) API_ARG(&c, key_times[first + i] > key_times[first + i - 1], "the key times of a channel are not strictly ascending");
    }
    // the nodes ordered by depth (a counting sort): the kernel's hierarchy pass takes them one level at a time
    levelStart.assign(levels + 1, 0);
    for (uint32_t n = 0; n < node_count; n++) levelStart[depth[n] + 1]++;
    for (uint32_t l = 0; l < levels; l++) levelStart[l + 1] += levelStart[l];
    std::vector<uint32_t> levelNodes(node_count), cursor(levelStart.begin(), levelStart.end() - 1);
    for (uint32_t n = 0; n < node_count; n++) levelNodes[cursor[depth[n]]++] = n;

    Packer pk;
    const size_t aParents = pk.add(parents, 4 * (size_t)node_count), aRest = pk.add(rest_trs, 40 * (size_t)node_count);
    const size_t aLevelNodes = pk.add(levelNodes.data(), 4 * (size_t)node_count), aLevelStart = pk.add(levelStart.data(), 4 * levelStart.size());
    const size_t aChannels = pk.add(channels, 8 * nch), aTimes = pk.add(key_times, 4 * (size_t)key_count), aValues = pk.add(key_values, 16 * (size_t)key_count);
    API_HIP(&c, hipSetDevice(c.device));
    AnimRig rig;
    API_HIP(&c, rig.dev.reserve(pk.bytes.size() + 16));
    API_HIP(&c, hipMemcpy(rig.dev.data(), pk.bytes.data(), pk.bytes.size(), hipMemcpyHostToDevice));
    const uint8_t* d = rig.dev.data();
    rig.view = AnimRigView{ (const int*)(d + aParents), (const float*)(d + aRest), (const uint32_t*)(d + aLevelNodes), (const uint32_t*)(d + aLevelStart),
                            (const uint2*)(d + aChannels), (const float*)(d + aTimes), (const float4*)(d + aValues), node_count, levels, clip_count, 0 };
    rig.durations.assign(durations, durations + clip_count);
    const uint64_t id = c.nextAnimId++;
    c.animRigs.emplace(id, std::move(rig));
    *out_rig = id;
    return PT_OK;
}

int pt_anim_release_rig(PtContext* ctx, uint64_t rig)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    Context& c = ctx->c;
    auto it = c.animRigs.find(rig);
    API_ARG(&c, it != c.animRigs.end(), "unknown rig id");
    API_ARG(&c, it->second.users == 0, "the rig is still referenced by an animated object");
    API_HIP(&c, hipSetDevice(c.device));
    API_HIP(&c, hipStreamSynchronize(c.stream));
    c.animRigs.erase(it);
    return PT_OK;
}

int pt_anim_create_object(PtContext* ctx, uint64_t rig, const float* transform16, uint32_t binding_count, const uint32_t* binding_nodes,
                          const uint32_t* binding_instances, const float* binding_globals16, uint32_t skin_count, const uint32_t* skin_mesh_nodes,
                          const uint32_t* skin_joint_counts, const uint32_t* joint_nodes, const float* inverse_binds16, uint64_t* out_object)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    Context& c = ctx->c;
    API_ARG(&c, out_object && transform16, "out_object / transform16 is NULL");
    auto rit = c.animRigs.find(rig);
    API_ARG(&c, rit != c.animRigs.end(), "unknown rig id");
    const uint32_t nodes = rit->second.view.nodeCount;
    API_ARG(&c, binding_count <= (1u << 20) && skin_count <= (1u << 16), "too many bindings / skins");
    API_ARG(&c, binding_count == 0 || (binding_nodes && binding_instances && binding_globals16), "a binding array is NULL");
    API_ARG(&c, skin_count == 0 || (skin_mesh_nodes && skin_joint_counts), "a skin array is NULL");
    API_ARG(&c, all_finite(transform16, 16) && all_finite(binding_globals16, 16 * (size_t)binding_count), "a transform is not finite");
    uint32_t maxInstance = 0;
    for (uint32_t b = 0; b < binding_count; b++) {
        API_ARG(&c, binding_nodes[b] == kNoNode || binding_nodes[b] < nodes, "a binding's node index is out of range");
        for (uint32_t k = 0; k < b; k++) API_ARG(&c, binding_instances[k] != binding_instances[b], "two bindings name the same instance");
        maxInstance = std::max(maxInstance, binding_instances[b]);
    }
    std::vector<uint32_t> firstJoint(skin_count + 1, 0), jointSkin;
    for (uint32_t s = 0; s < skin_count; s++) {
        API_ARG(&c, skin_mesh_nodes[s] == kNoNode || skin_mesh_nodes[s] < nodes, "a skin's mesh-node index is out of range");
        API_ARG(&c, skin_joint_counts[s] <= 65536u, "a skin has more than 65536 joints");      // the skeletal vertex names joints with 16 bits
        firstJoint[s + 1] = firstJoint[s] + skin_joint_counts[s];
        jointSkin.insert(jointSkin.end(), skin_joint_counts[s], s);
    }
    const uint32_t joints = firstJoint[skin_count];
    API_ARG(&c, joints == 0 || (joint_nodes && inverse_binds16), "joint_nodes / inverse_binds16 is NULL");
    for (uint32_t j = 0; j < joints; j++) API_ARG(&c, joint_nodes[j] == kNoNode || joint_nodes[j] < nodes, "a joint's node index is out of range");
    API_ARG(&c, all_finite(inverse_binds16, 16 * (size_t)joints), "an inverse bind matrix is not finite");

    Packer pk;
    const size_t aView = pk.add(nullptr, sizeof(AnimObjectView));
    const size_t aGlobals = pk.add(nullptr, 64 * (size_t)nodes), aSkeletal = pk.add(nullptr, 48 * (size_t)joints), aInverse = pk.add(nullptr, 64 * (size_t)skin_count);
    const size_t aBNodes = pk.add(binding_nodes, 4 * (size_t)binding_count), aBInst = pk.add(binding_instances, 4 * (size_t)binding_count);
    const size_t aBGlobals = pk.add(binding_globals16, 64 * (size_t)binding_count);
    const size_t aSNodes = pk.add(skin_mesh_nodes, 4 * (size_t)skin_count);
    const size_t aJNodes = pk.add(joint_nodes, 4 * (size_t)joints), aJSkin = pk.add(jointSkin.data(), 4 * (size_t)joints), aIB = pk.add(inverse_binds16, 64 * (size_t)joints);
    API_HIP(&c, hipSetDevice(c.device));
    AnimObject obj;
    API_HIP(&c, obj.dev.reserve(pk.bytes.size() + 16));
    uint8_t* d = obj.dev.data();
    AnimObjectView v{};
    v.rig = rit->second.view;
    memcpy(v.transform, transform16, 64);
    v.globals = (float*)(d + aGlobals); v.skeletal = (float*)(d + aSkeletal); v.skinInverse = (float*)(d + aInverse);
    v.bindingNodes = (const uint32_t*)(d + aBNodes); v.bindingInstances = (const uint32_t*)(d + aBInst); v.bindingGlobals = (const float*)(d + aBGlobals);
    v.skinMeshNodes = (const uint32_t*)(d + aSNodes);
    v.jointNodes = (const uint32_t*)(d + aJNodes); v.jointSkin = (const uint32_t*)(d + aJSkin); v.inverseBinds = (const float*)(d + aIB);
    v.bindingCount = binding_count; v.skinCount = skin_count; v.jointCount = joints;
    memcpy(pk.bytes.data() + aView, &v, sizeof v);                 // (globals, skeletal and inverses start as zeros)
    API_HIP(&c, hipMemcpy(d, pk.bytes.data(), pk.bytes.size(), hipMemcpyHostToDevice));
    obj.rig = rig; obj.viewDev = (const AnimObjectView*)(d + aView); obj.globals = v.globals; obj.skeletal = v.skeletal;
    obj.nodeCount = nodes; obj.maxInstance = maxInstance; obj.hasBindings = binding_count != 0; obj.skinFirstJoint = std::move(firstJoint);
    rit->second.users++;
    const uint64_t id = c.nextAnimId++;
    c.animObjects.emplace(id, std::move(obj));
    *out_object = id;
    return PT_OK;
}

int pt_anim_release_object(PtContext* ctx, uint64_t object)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    Context& c = ctx->c;
    auto it = c.animObjects.find(object);
    API_ARG(&c, it != c.animObjects.end(), "unknown animated-object id");
    API_HIP(&c, hipSetDevice(c.device));
    API_HIP(&c, hipStreamSynchronize(c.stream));
    auto rit = c.animRigs.find(it->second.rig);
    if (rit != c.animRigs.end() && rit->second.users) rit->second.users--;
    c.animObjects.erase(it);
    return PT_OK;
}

int pt_anim_evaluate(PtContext* ctx, const struct PtAnimState* states, uint32_t count, PtInstanceData* device_instances)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    Context& c = ctx->c;
    API_ARG(&c, states || count == 0, "states is NULL");
    API_ARG(&c, !device_instances || device_instances == c.instanceData, "device_instances must be the array bound with pt_set_instance_data");
    if (!count) return PT_OK;
    // check everything first: a refused call changes nothing
    const uint64_t stamp = ++c.animStamp;
    for (uint32_t i = 0; i < count; i++) {
        auto it = c.animObjects.find(states[i].Object);
        API_ARG(&c, it != c.animObjects.end(), "unknown animated-object id");
        AnimObject& o = it->second;
        API_ARG(&c, o.stamp != stamp, "an animated object is named twice in one pt_anim_evaluate");
        o.stamp = stamp;
        API_ARG(&c, states[i].Clip < c.animRigs.at(o.rig).view.clipCount, "clip index out of range");
        API_ARG(&c, std::isfinite(states[i].Time), "Time is not finite");
        API_ARG(&c, !device_instances || !o.hasBindings || o.maxInstance < c.instanceDataCount, "a binding's instance index is beyond the bound instance data");
    }
    API_HIP(&c, hipSetDevice(c.device));
    API_HIP(&c, grow(c.stream, nullptr, want(c.animStatesDev, count > c.animStatesDev.capacity() ? (size_t)count * 2 : 0)));   // head room
    Context::UploadStage& sg = c.animStage[c.animStageNext];
    if (sg.event) API_HIP(&c, hipEventSynchronize(sg.event.get()));    // the copy that last read this buffer has run
    else API_HIP(&c, create_event(sg.event, hipEventDisableTiming));
    const size_t bytes = sizeof(AnimStateDev) * (size_t)count;
    if (bytes > sg.host.capacity()) {                                  // (the event, not the stream, guards it: a fresh one, moved in)
        PinnedBuffer<uint8_t> fresh;
        API_HIP(&c, fresh.reserve(bytes * 2));
        sg.host = std::move(fresh);
    }
    AnimStateDev* h = (AnimStateDev*)sg.host.data();
    for (uint32_t i = 0; i < count; i++) {
        const AnimObject& o = c.animObjects.at(states[i].Object);
        const double duration = c.animRigs.at(o.rig).durations[states[i].Clip];
        h[i] = AnimStateDev{ o.viewDev, states[i].Clip, (device_instances && !o.evaluated) ? 1u : 0u, duration == 0.0 ? 0.0 : states[i].Time };
    }
    API_HIP(&c, hipMemcpyAsync(c.animStatesDev.data(), h, bytes, hipMemcpyHostToDevice, c.stream));
    API_HIP(&c, hipEventRecord(sg.event.get(), c.stream));
    c.animStageNext ^= 1u;
    k_anim_pose<<<count, kAnimLanes, 0, c.stream>>>(c.animStatesDev.data(), device_instances);
    API_HIP(&c, hipGetLastError());
    if (device_instances) for (uint32_t i = 0; i < count; i++) c.animObjects.at(states[i].Object).evaluated = true;
    return PT_OK;
}

int pt_anim_skeletal_transforms(PtContext* ctx, uint64_t object, uint32_t skin, const float** device_ptr, uint32_t* joint_count)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    Context& c = ctx->c;
    API_ARG(&c, device_ptr && joint_count, "device_ptr / joint_count is NULL");
    auto it = c.animObjects.find(object);
    API_ARG(&c, it != c.animObjects.end(), "unknown animated-object id");
    const AnimObject& o = it->second;
    API_ARG(&c, skin + 1 < o.skinFirstJoint.size(), "skin index out of range");
    *device_ptr = o.skeletal + 12 * (size_t)o.skinFirstJoint[skin];
    *joint_count = o.skinFirstJoint[skin + 1] - o.skinFirstJoint[skin];
    return PT_OK;
}

int pt_anim_download_globals(PtContext* ctx, uint64_t object, float* host_dst16, uint32_t capacity, uint32_t* out_count)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    Context& c = ctx->c;
    API_ARG(&c, out_count && (host_dst16 || capacity == 0), "out_count / host_dst16 is NULL");
    auto it = c.animObjects.find(object);
    API_ARG(&c, it != c.animObjects.end(), "unknown animated-object id");
    return download_counted(c, it->second.globals, it->second.nodeCount, 16, host_dst16, capacity > 0x0FFFFFFFu ? 0xFFFFFFFFu : capacity * 16u, out_count);
}

int pt_anim_download_skeletal(PtContext* ctx, uint64_t object, uint32_t skin, float* host_dst12, uint32_t capacity, uint32_t* out_count)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    Context& c = ctx->c;
    API_ARG(&c, out_count && (host_dst12 || capacity == 0), "out_count / host_dst12 is NULL");
    auto it = c.animObjects.find(object);
    API_ARG(&c, it != c.animObjects.end(), "unknown animated-object id");
    const AnimObject& o = it->second;
    API_ARG(&c, skin + 1 < o.skinFirstJoint.size(), "skin index out of range");
    return download_counted(c, o.skeletal + 12 * (size_t)o.skinFirstJoint[skin], o.skinFirstJoint[skin + 1] - o.skinFirstJoint[skin], 12, host_dst12,
                            capacity > 0x0FFFFFFFu ? 0xFFFFFFFFu : capacity * 12u, out_count);
}

int pt_anim_debug_slerp(PtContext* ctx, const float* q0, const float* q1, const float* t, uint32_t n, float* out)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    Context& c = ctx->c;
    API_ARG(&c, n == 0 || (q0 && q1 && t && out), "an array is NULL");
    API_ARG(&c, n <= (1u << 20), "at most 2^20 cases");
    if (!n) return PT_OK;
    API_HIP(&c, hipSetDevice(c.device));
    DeviceBuffer<float> in, res;
    API_HIP(&c, in.reserve(9 * (size_t)n));
    API_HIP(&c, res.reserve(12 * (size_t)n));
    API_HIP(&c, hipStreamSynchronize(c.stream));
    API_HIP(&c, hipMemcpy(in.data(), q0, 16 * (size_t)n, hipMemcpyHostToDevice));
    API_HIP(&c, hipMemcpy(in.data() + 4 * (size_t)n, q1, 16 * (size_t)n, hipMemcpyHostToDevice));
    API_HIP(&c, hipMemcpy(in.data() + 8 * (size_t)n, t, 4 * (size_t)n, hipMemcpyHostToDevice));
    k_anim_debug_slerp<<<(n + 255u) / 256u, 256, 0, c.stream>>>((const float4*)in.data(), (const float4*)(in.data() + 4 * (size_t)n), in.data() + 8 * (size_t)n, n, res.data());
    API_HIP(&c, hipGetLastError());
    API_HIP(&c, hipStreamSynchronize(c.stream));
    API_HIP(&c, hipMemcpy(out, res.data(), 48 * (size_t)n, hipMemcpyDeviceToHost));
    return PT_OK;
}

} // extern "C"
