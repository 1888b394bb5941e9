// pt_di.hip -- direct lighting over emissive triangles (gfx950): light preparation and the DI pass.
//
//   k_light_count / k_light_fill   <- the task table of Shaders/LightPreparation.hlsl (FindTask) and Source/LightPreparation.ixx:
//                                     the scene's emissive triangles, ordered by instance, geometry, triangle
//   k_light_records                <- LightPreparation.hlsl main: TriangleLight::Initialize (Light.hlsli) on the world-space
//                                     vertices, CalculatePower; run at every render (moving instances, refits)
//   k_cdf_*                        <- the local-light pdf texture of the reference's Power_RIS mode, as a fixed-order prefix sum
//   k_di_presample_tiles           <- LocalLightPresampling.hlsl: the Power_RIS light tiles (POWER_RIS, REGIR_RIS)
//   k_pdf_level0 / k_pdf_denominator / k_di_presample_tiles_mip <- the LocalLightPDF texture of App::PrepareReSTIRDI (pt_di_set_pdf_mipmap): level 0 on
//                                     the Z-curve, its chain by pt_mip.hip, and the tiles by a descent of the chain instead of the prefix sum
//   k_di_regir_build               <- ReGIRPresampling.hlsl, Grid mode: the ReGIR cells (REGIR_RIS)
//   k_di_regir_build_onion         <- the same over the Onion layout's cells (pt_di_set_regir_layout; the reference's compiled mode)
//   k_di<Source>                   <- DIInitialSampling (local lights only, streaming RIS) + DIFinalShading, no temporal /
//                                     spatial reuse (RTXDIAppBridge.hlsli RAB_GetGBufferSurface, RAB_Surface::Shade, GetFinalVisibility)
//   k_di_initial_temporal<..., VIS, Source> <- DIInitialSampling + DITemporalResampling (boiling filter), with reservoir reuse on
//   k_di_spatial_shade<..., VIS>   <- DISpatialResampling + DIFinalShading
//   both with BIAS = kDIBiasPairwise <- pairwise-MIS bias correction (pt_di_set_pairwise): one pass over the neighbours, no rays
//   both with VIS != 0             <- the same with visibility in the reservoirs (pt_di_set_visibility):
//                                     initial visibility (DIInitialSampling.hlsl:49-54), Raytraced bias correction
//                                     (RAB_GetConservativeVisibility / RAB_GetTemporalConservativeVisibility), the final-visibility store and
//                                     reuse and discardInvisibleSamples (DIFinalShading.hlsl:32-56)
//   k_di_brdf_rays                 <- the BRDF candidates of initial sampling (pt_di_set_brdf_sampling): one all-lobe BSDF sample and one
//                                     closest-hit walk per pixel and candidate, a 16-byte record each; k_di and k_di_initial_temporal with
//                                     BRDF = true read the records and weight light and BRDF candidates by MIS
// Source is where initial sampling draws its candidates from: DIPowerCDF (the prefix sum, the default) or DISampling (Uniform,
// Power_RIS, ReGIR). Every kernel reads its surfaces with di_surface, draws with di_initial and shades with di_shadow_ray +
// di_final_write.
// DESIGN.md section 1 ("Direct lighting") is the arithmetic spec: seeding, draw order, triangle mapping.
#include "pt_internal.hpp"

#include <cassert>
#include <cmath>
#include <cstring>
#include <type_traits>

#include "pt_shade.hpp"

namespace pt {

constexpr uint32_t kDISalt = 0x44490001u;            // the DI pass's own stream: seed = ml_hash(rng_init(x, y, FrameIndex) ^ kDISalt)
constexpr uint32_t kScanBlock = 1024u;               // lights per block of the prefix sum (256 threads x 4)
constexpr uint32_t kLightRec16 = sizeof(PtTriangleLight) / 16u;
static_assert(sizeof(PtTriangleLight) == 80, "layout");

// ---- light list ------------------------------------------------------------------------------
PT_DEV bool emissive(const PtMaterial& m) { const v3 e = material_emission(m); return e.x > 0.0f || e.y > 0.0f || e.z > 0.0f; }
PT_DEV uint32_t geometry_triangles(const PtObjectData& od, const HeapEntry* heap)
{
    const HeapEntry ib = heap[od.MeshDescriptors.Indices];
    return ib.stride ? (uint32_t)(ib.bytes / ib.stride / 3u) : 0u;
}

// one block: emissive triangles per instance (hidden instances: none), exclusive prefix sum in instance order; start[n] = total
__global__ __launch_bounds__(1024) void k_light_count(const InstanceSource* __restrict__ src, const BlasEntry* __restrict__ table, uint32_t n,
                                                      const PtObjectData* __restrict__ objects, const HeapEntry* __restrict__ heap, uint32_t* __restrict__ start)
{
    __shared__ uint32_t part[1024];
    uint32_t carry = 0;
    for (uint32_t base = 0; base < n; base += 1024u) {
        const uint32_t i = base + threadIdx.x;
        uint32_t cnt = 0;
        if (i < n && src[i].mask != 0u) {
            const BlasEntry b = table[src[i].blasSlot];
            for (uint32_t g = 0; g < b.geometryCount; g++) {
                const PtObjectData& od = objects[src[i].instanceID + g];
                if (emissive(od.Material)) cnt += geometry_triangles(od, heap);
            }
        }
        part[threadIdx.x] = cnt;
        __syncthreads();
        for (uint32_t off = 1; off < 1024u; off <<= 1) {            // inclusive scan (integers: exact in any order)
            const uint32_t v = threadIdx.x >= off ? part[threadIdx.x - off] : 0u;
            __syncthreads();
            part[threadIdx.x] += v;
            __syncthreads();
        }
        if (i < n) start[i] = carry + part[threadIdx.x] - cnt;
        carry += part[1023];
        __syncthreads();
    }
    if (threadIdx.x == 0) start[n] = carry;
}

// one block per instance: its emissive triangles in (geometry, triangle) order. first[object]: the list entry of the object's triangle 0
// (the table is ~0u before the pass; instances that share an InstanceID leave the smallest entry)
__global__ __launch_bounds__(256) void k_light_fill(const InstanceSource* __restrict__ src, const BlasEntry* __restrict__ table, const PtObjectData* __restrict__ objects,
                                                    const HeapEntry* __restrict__ heap, const uint32_t* __restrict__ start, uint4* __restrict__ list,
                                                    uint32_t* __restrict__ first, uint32_t objectCount)
{
    const uint32_t i = blockIdx.x;
    if (src[i].mask == 0u) return;
    const BlasEntry b = table[src[i].blasSlot];
    uint32_t at = start[i];
    for (uint32_t g = 0; g < b.geometryCount; g++) {
        const uint32_t o = src[i].instanceID + g;
        if (!emissive(objects[o].Material)) continue;
        const uint32_t nt = geometry_triangles(objects[o], heap);
        for (uint32_t t = threadIdx.x; t < nt; t += 256u) list[at + t] = make_uint4(i, g, t, o);
        if (threadIdx.x == 0 && o < objectCount) atomicMin(&first[o], at);
        at += nt;
    }
}

// ---- per-render records (PtTriangleLight, 5 x 16 B) -------------------------------------------
PT_DEV v3 load_position(const HeapEntry& vb, uint32_t stride, uint32_t vi)
{
    const uint64_t at = (uint64_t)stride * vi;
    if (at + 12u > vb.bytes) return V3(0.0f, 0.0f, 0.0f);             // an index beyond the vertex buffer reads nothing
    const PT_GLOBAL_AS float* p = gptr<float>((const uint8_t*)vb.ptr + at);
    return V3(p[0], p[1], p[2]);
}
PT_DEV v3 affine(const float* M, v3 p)                                  // Geometry::AffineTransform with a row-major 3x4
{
    return V3(M[0] * p.x + M[1] * p.y + M[2] * p.z + M[3], M[4] * p.x + M[5] * p.y + M[6] * p.z + M[7], M[8] * p.x + M[9] * p.y + M[10] * p.z + M[11]);
}

__global__ __launch_bounds__(256) void k_light_records(const uint4* __restrict__ list, uint32_t count, const InstanceSource* __restrict__ src, const PtObjectData* __restrict__ objects,
                                                       const HeapEntry* __restrict__ heap, const HeapEntry* __restrict__ shadeTex, const float* __restrict__ srgbLut,
                                                       float4* __restrict__ rec, float* __restrict__ power)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= count) return;
    const uint4 e = list[k];
    const PtObjectData& od = objects[e.w];
    const HeapEntry vb = heap[od.MeshDescriptors.Vertices], ib = heap[od.MeshDescriptors.Indices];
    const uint32_t stride = od.VertexDesc.Stride;
    uint32_t vi[3];
    for (int j = 0; j < 3; j++) vi[j] = load_index_dev(ib.ptr, ib.stride, 3u * e.z + j);
    float M[12];
    for (int j = 0; j < 12; j++) M[j] = src[e.x].transform[j];
    const v3 p0 = affine(M, load_position(vb, stride, vi[0])), p1 = affine(M, load_position(vb, stride, vi[1])), p2 = affine(M, load_position(vb, stride, vi[2]));
    const v3 e0 = p1 - p0, e1 = p2 - p0;
    const v3 nrm = cross(e0, e1);
    const float len = sqrtf(dot(nrm, nrm));
    v3 n = V3(0.0f, 0.0f, 0.0f); float area = 0.0f;
    if (len > 0.0f) { n = V3(nrm.x / len, nrm.y / len, nrm.z / len); area = len / 2.0f; }
    v3 L = material_emission(od.Material);
    // the emissive texture at the UV centroid, bilinear mip 0 (the reference: SampleGrad over the triangle's UV footprint)
    const HeapEntry t = shadeTex[(size_t)e.w * kTextureSlots + TEX_EmissiveColor];
    if (t.ptr && (L.x > 0.0f || L.y > 0.0f || L.z > 0.0f)) {
        const uint32_t off = od.VertexDesc.AttributeOffsets.TextureCoordinates[t.kind & 1u];
        float uv[2] = { 0.0f, 0.0f };
        if (off != ~0u) {
            float a[3][2];
            for (int j = 0; j < 3; j++) {
                const uint64_t at = (uint64_t)stride * vi[j] + off;
                a[j][0] = a[j][1] = 0.0f;
                if (at + 4u <= vb.bytes) { const PT_GLOBAL_AS uint16_t* q = gptr<uint16_t>((const uint8_t*)vb.ptr + at); a[j][0] = f16_to_f32(q[0]); a[j][1] = f16_to_f32(q[1]); }
            }
            for (int c = 0; c < 2; c++) uv[c] = (a[0][c] + a[1][c] + a[2][c]) / 3.0f;
        }
        const f4 s = texture_sample(t, srgbLut, uv[0], uv[1]);
        L = V3(L.x * s.x, L.y * s.y, L.z * s.z);
    }
    const float pw = area * kPi * ml_luminance(L);
    float4* r = rec + kLightRec16 * (size_t)k;
    r[0] = make_float4(p0.x, p0.y, p0.z, area);
    r[1] = make_float4(e0.x, e0.y, e0.z, pw);
    r[2] = make_float4(e1.x, e1.y, e1.z, __uint_as_float(e.x));
    r[3] = make_float4(n.x, n.y, n.z, __uint_as_float(e.z));
    r[4] = make_float4(L.x, L.y, L.z, __uint_as_float(e.y));
    power[k] = pw;
}

// ---- sampling table: inclusive prefix sum of the powers in a fixed order (bit-identical from run to run) ----------------------
// local: each block sums kScanBlock lights (4 per thread, sequentially, then a Hillis-Steele scan of the 256 thread sums)
__global__ __launch_bounds__(256) void k_cdf_local(const float* __restrict__ power, uint32_t count, float* __restrict__ cdf, float* __restrict__ blockSums)
{
    __shared__ float part[256];
    const uint32_t b0 = blockIdx.x * kScanBlock + threadIdx.x * 4u;
    float v[4], s = 0.0f;
    for (int j = 0; j < 4; j++) { v[j] = b0 + j < count ? power[b0 + j] : 0.0f; s += v[j]; v[j] = s; }
    part[threadIdx.x] = s;
    __syncthreads();
    for (uint32_t off = 1; off < 256u; off <<= 1) {
        const float a = threadIdx.x >= off ? part[threadIdx.x - off] : 0.0f;
        __syncthreads();
        part[threadIdx.x] += a;
        __syncthreads();
    }
    const float before = threadIdx.x ? part[threadIdx.x - 1] : 0.0f;
    for (int j = 0; j < 4; j++) if (b0 + j < count) cdf[b0 + j] = before + v[j];
    if (threadIdx.x == 255) blockSums[blockIdx.x] = part[255];
}
// one thread: running offsets of the blocks, in block order; blockSums[nb] = the total
__global__ void k_cdf_blocks(float* __restrict__ blockSums, uint32_t nb)
{
    float s = 0.0f;
    for (uint32_t b = 0; b < nb; b++) { const float t = blockSums[b]; blockSums[b] = s; s += t; }
    blockSums[nb] = s;
}
// adds the block offsets; the last entry becomes the total itself (the order of the sums above can leave them an ulp apart, and the
// selection rule needs cdf[count - 1] == total so that a light past the last positive power can never be returned)
__global__ __launch_bounds__(256) void k_cdf_add(float* __restrict__ cdf, uint32_t count, const float* __restrict__ blockSums, uint32_t nb)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k + 1u == count) cdf[k] = blockSums[nb];
    else if (k < count && k >= kScanBlock) cdf[k] = blockSums[k / kScanBlock] + cdf[k];
}

// ---- the DI pass ----------------------------------------------------------------------------------------------------------
// G-buffer planes a surface is read from (the current frame's, or the Previous* textures)
struct DIGBuffer { const void *depth, *normalRoughness, *geometricNormal, *baseColorMetalness, *ior, *transmission; };
// what names a frame: its G-buffer and camera (the current one, or PreviousProjectionToView / PreviousViewToWorld / PreviousPosition)
struct DIView { DIGBuffer g; float position[3], projectionToView[16], viewToWorld[16]; };
struct DIArgs {
    FrameView fv; PtTextures tx; DIView view; float jitter[2];
    const float4* lights; const float* cdf; const float* total; uint32_t count;
    uint32_t frameIndex, samples, denoiser, lastPass, ext;
    // BRDF candidates (pt_di_set_brdf_sampling); read only by the BRDF instantiations
    const uint4* brdfRecords; const uint32_t* firstLight; uint32_t brdfSamples, objectCount; float brdfCutoff;   // firstLight[objectCount]
};

// first light whose inclusive prefix exceeds x: a light of zero power never qualifies. x >= total (rounding of u * total): the
// first light that reaches the total, which has power > 0.
PT_DEV uint32_t select_light(const float* __restrict__ cdf, uint32_t n, float x, float total)
{
    const float t = x < total ? x : total;
    uint32_t lo = 0, hi = n - 1u;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        const float c = cdf[mid];
        if (x < total ? c > t : c >= t) hi = mid; else lo = mid + 1u;
    }
    return lo;
}

// Shade(lightSample) of RAB_Surface, RTXDIAppBridge.hlsli: all-lobe Evaluate times radiance / solid-angle pdf
// pdf: the all-lobe EvaluatePDF of the direction (the BRDF candidates' MIS weight reads it; 0 where nothing is evaluated)
PT_DEV void shade_sample(const BSDFSample& bs, const SurfaceVectors& svec, const float w[3], uint32_t ext, v3 P, v3 V, v3 pos, v3 Le, float pdfSA, v3& dif, v3& spc, float& pdf)
{
    dif = V3(0.0f, 0.0f, 0.0f); spc = V3(0.0f, 0.0f, 0.0f); pdf = 0.0f;
    if (!(pdfSA > 0.0f)) return;
    bs.EvaluateAll(svec, normalize(pos - P), V, w, pdf, dif, spc, ext);
    const float inv = 1.0f / pdfSA;
    dif = V3(dif.x * Le.x * inv, dif.y * Le.y * inv, dif.z * Le.z * inv);
    spc = V3(spc.x * Le.x * inv, spc.y * Le.y * inv, spc.z * Le.z * inv);
}

struct DISurface { v3 P, V; SurfaceVectors svec; BSDFSample bs; float w[3]; float depth; };

// RAB_GetGBufferSurface (RTXDIAppBridge.hlsli:293-345) of a view at pixel (x, y); false: the empty surface. The jitter is the current
// frame's whichever the view (:332).
PT_DEV bool di_surface(const DIArgs& a, const DIView& view, size_t pi, uint32_t x, uint32_t y, DISurface& s)
{
    const DIGBuffer& g = view.g;
    const float depth = ((const float*)g.depth)[pi];
    if (!isfinite(depth)) return false;
    const short4 nr = ((const short4*)g.normalRoughness)[pi];
    const float roughness = snorm16_to_f32(nr.w);
    if (roughness < 0.05f) return false;                                 // MinRoughness
    const float u = ((float)x + 0.5f + a.jitter[0]) / (float)a.fv.width, v = ((float)y + 0.5f + a.jitter[1]) / (float)a.fv.height;
    float q[4];
    xform4(view.projectionToView, V3(u * 2.0f + -1.0f, v * -2.0f + 1.0f, 0.5f), q);     // Camera::ReconstructWorldPosition
    const v3 vp = V3(q[0] / q[2] * depth, q[1] / q[2] * depth, depth);
    xform4(view.viewToWorld, vp, q);
    s.P = V3(q[0], q[1], q[2]);
    s.V = normalize(V3(view.position[0] - s.P.x, view.position[1] - s.P.y, view.position[2] - s.P.z));
    const short2 ge = ((const short2*)g.geometricNormal)[pi];
    const v3 gn = oct_decode(snorm16_to_f32(ge.x), snorm16_to_f32(ge.y));
    const bool front = dot(gn, s.V) > 0.0f;
    s.svec = surface_vectors(front, gn, V3(snorm16_to_f32(nr.x), snorm16_to_f32(nr.y), snorm16_to_f32(nr.z)));
    const uchar4 bcm = ((const uchar4*)g.baseColorMetalness)[pi];
    const float metal = unorm8_to_f32(bcm.w);
    const float tr = metal < 1.0f ? unorm8_to_f32(((const uint8_t*)g.transmission)[pi]) : 0.0f;
    s.bs.Initialize(V3(unorm8_to_f32(bcm.x), unorm8_to_f32(bcm.y), unorm8_to_f32(bcm.z)), metal, roughness, f16_to_f32(((const uint16_t*)g.ior)[pi]), tr, front);
    s.bs.ComputeLobeWeights(s.svec, s.V, a.ext, s.w);
    s.depth = depth;
    return true;
}

// p-hat of light sample (li, U, V) at surface s (RAB_GetLightSampleTargetPdfForSurface): the luminance of the all-lobe Shade. The
// sample's point is re-derived from the light record: Math::SampleTriangle with r1 = U, r2 = V. power: the record's Power.
// mis (BRDF candidates): the sample's solid-angle pdf, its all-lobe BSDF pdf and its distance.
struct DIMisTerms { float pdfSA, pdfBrdf, dist; };
PT_DEV float di_target(const DIArgs& a, const DISurface& s, uint32_t li, float U, float V, v3& pos, v3& dif, v3& spc, float& power, DIMisTerms* mis = nullptr)
{
    const float4* L = a.lights + kLightRec16 * (size_t)li;
    const float4 l0 = L[0], l1 = L[1], l2 = L[2], l3 = L[3], l4 = L[4];
    const float sq = sqrtf(U);                                          // Math::SampleTriangle
    const float b0 = sq * (1.0f - V), b1 = sq * V;
    pos = V3(l0.x + l1.x * b0 + l2.x * b1, l0.y + l1.y * b0 + l2.y * b1, l0.z + l1.z * b0 + l2.z * b1);
    const v3 d = pos - s.P;
    const float len = sqrtf(dot(d, d));
    const v3 dn = V3(d.x / len, d.y / len, d.z / len);
    const float cosL = fabsf(dot(dn, -V3(l3.x, l3.y, l3.z)));
    const float pdfSA = (1.0f / l0.w) * len * len / cosL;              // CalculateSolidAnglePDF
    float pdfBrdf;
    shade_sample(s.bs, s.svec, s.w, a.ext, s.P, s.V, pos, V3(l4.x, l4.y, l4.z), pdfSA, dif, spc, pdfBrdf);
    power = l1.w;
    if (mis) { mis->pdfSA = pdfSA; mis->pdfBrdf = pdfBrdf; mis->dist = len; }
    return ml_luminance(dif + spc);
}

// ---- local-light sampling (pt_di_set_light_sampling; DESIGN.md section 1, "Local-light sampling") ------------------------------------
// The RTXDI SDK's static parameters. The SDK is not in the reference tree: these are its defaults from memory, unpinned.
constexpr uint32_t kDITileCount = 128u, kDITileSize = 1024u;       // Power_RIS: light tiles x entries
constexpr uint32_t kDIScreenTile = 16u;                            // pixels per side of the screen tile that shares one light tile
constexpr uint32_t kDIGrid = 16u, kDICellLights = 512u;            // ReGIR Grid mode: cells per axis, lights per cell
constexpr float kDIJitterScale = 2.0f;                             // max(0, 2 * samplingJitter) with jitter 1 (RTXDI.ixx:93)
constexpr uint32_t kDITileEntries = kDITileCount * kDITileSize, kDICellEntries = kDIGrid * kDIGrid * kDIGrid * kDICellLights;
constexpr uint32_t kDIPresampleSalt = 0x44490004u, kDIReGIRSalt = 0x44490005u, kDIReGIRCoherentSalt = 0x44490006u, kDIScreenTileSalt = 0x44490007u;
static_assert(sizeof(PtDILightSamplingSettings) == 16 && sizeof(PtDIPresampledLight) == 8, "layout");

// Power_RIS presampling (LocalLightPresampling.hlsl): one entry per thread, a power-proportional light from the prefix sum and its
// inverse selection pdf. Seeded as ReGIRPresampling.hlsl splits its index: (g & 0xfff, g >> 12).
__global__ __launch_bounds__(256) void k_di_presample_tiles(const float4* __restrict__ lights, const float* __restrict__ cdf, const float* __restrict__ total,
                                                            uint32_t count, uint32_t frameIndex, uint2* __restrict__ tiles)
{
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= kDITileEntries) return;
    const float t = *total;
    uint2 e = make_uint2(~0u, 0u);
    if (t > 0.0f && isfinite(t)) {
        uint32_t rng = ml_hash(rng_init(g & 0xFFFu, g >> 12, frameIndex) ^ kDIPresampleSalt);
        const uint32_t li = select_light(cdf, count, rng_float(rng) * t, t);
        e = make_uint2(li, __float_as_uint(t / lights[kLightRec16 * (size_t)li + 1].w));
    }
    tiles[g] = e;
}

// ---- the local-light PDF texture (pt_di_set_pdf_mipmap; DESIGN.md section 1, "Local-light PDF texture") ------------------------------
// the inverse of RTXDI_LinearIndexToZCurve: x gives the even bits of the index, y the odd ones
PT_DEV uint32_t di_z_spread(uint32_t v)
{
    v &= 0x0000FFFFu; v = (v | (v << 8)) & 0x00FF00FFu; v = (v | (v << 4)) & 0x0F0F0F0Fu; v = (v | (v << 2)) & 0x33333333u; v = (v | (v << 1)) & 0x55555555u;
    return v;
}
PT_DEV uint32_t di_z_index(uint32_t x, uint32_t y) { return di_z_spread(x) | (di_z_spread(y) << 1); }

// Level 0, one thread per texel: Power of the light whose Z-curve position the texel is, 0 where there is none (the reference clears the
// texture and LightPreparation.hlsl:133 scatters; a gather needs no clear)
__global__ __launch_bounds__(256) void k_pdf_level0(const float* __restrict__ power, uint32_t count, uint32_t width, uint32_t texels, float* __restrict__ level0)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= texels) return;
    const uint32_t li = di_z_index(i & (width - 1u), i / width);           // the width is a power of two
    level0[i] = li < count ? power[li] : 0.0f;
}
// one thread: what the source pdf of a light divides its Power by, top * M * M (RAB_EvaluateLocalLightSourcePdf); M is a power of two
__global__ void k_pdf_denominator(const float* __restrict__ top, float M, float* __restrict__ out) { *out = (*top * M) * M; }

// Power_RIS presampling by a descent of the chain (RTXDI_PresampleLocalLights over RTXDI_SamplePdfMipmap): the entry's stream is the one of
// k_di_presample_tiles, one draw per level. pdf: the levels back to back, level 0 first, `texels` floats in all.
__global__ __launch_bounds__(256) void k_di_presample_tiles_mip(const float* __restrict__ pdf, uint32_t width, uint32_t height, uint32_t mips, uint32_t texels,
                                                                uint32_t count, uint32_t frameIndex, uint2* __restrict__ tiles)
{
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= kDITileEntries) return;
    uint32_t rng = ml_hash(rng_init(g & 0xFFFu, g >> 12, frameIndex) ^ kDIPresampleSalt);
    uint32_t px = 0, py = 0;
    float p = 1.0f;
    bool empty = false;
    uint32_t at = mips >= 2u ? texels - 1u : texels;                       // where the level above the first one read starts
    for (int level = mips >= 2u ? (int)mips - 2 : 0; level >= 0; level--) {
        const uint32_t lw = max(1u, width >> level), lh = max(1u, height >> level);
        at -= lw * lh;
        px *= 2u; py *= 2u;
        const float* L = pdf + at;
        auto texel = [&](uint32_t x, uint32_t y) { const float t = x < lw && y < lh ? L[(size_t)y * lw + x] : 0.0f; return t > 0.0f ? t : 0.0f; };   // max(0, NaN) = 0
        const float s0 = texel(px, py), s1 = texel(px, py + 1u), s2 = texel(px + 1u, py), s3 = texel(px + 1u, py + 1u);
        const float sum = ((s0 + s1) + s2) + s3;
        if (!(sum > 0.0f && isfinite(sum))) { empty = true; break; }
        const float p0 = s0 / sum, p1 = s1 / sum, p2 = s2 / sum, p3 = s3 / sum;
        float r = rng_float(rng);
        if (r < p0) p *= p0;
        else {
            r -= p0;
            if (r < p1) { py += 1u; p *= p1; }
            else {
                r -= p1;
                if (r < p2) { px += 1u; p *= p2; }
                else { px += 1u; py += 1u; p *= p3; }
            }
        }
    }
    const uint32_t li = di_z_index(px, py);
    tiles[g] = !empty && p > 0.0f && li < count ? make_uint2(li, __float_as_uint(1.0f / p)) : make_uint2(~0u, 0u);
}

// TriangleLight::CalculateWeightForVolume with CalculateAverageDistanceToVolume (Light.hlsli:16-24, 84-95)
PT_DEV float di_volume_weight(const float4* L, v3 c, float radius)
{
    const float4 l0 = L[0], l1 = L[1], l2 = L[2], l3 = L[3], l4 = L[4];
    const v3 base = V3(l0.x, l0.y, l0.z);
    if (dot(c - base, V3(l3.x, l3.y, l3.z)) < -radius) return 0.0f;
    const v3 d = V3(base.x + (l1.x + l2.x) / 3.0f, base.y + (l1.y + l2.y) / 3.0f, base.z + (l1.z + l2.z) / 3.0f) - c;
    const float dc = sqrtf(dot(d, d));
    const float value = dc + radius * 1.1547f;
    const float dist = dc + radius * radius * radius / (value * value);
    return fminf(l0.w / (dist * dist), 2.0f * kPi) * ml_luminance(V3(l4.x, l4.y, l4.z));
}

// One slot of a ReGIR cell (ReGIRPresampling.hlsl): BuildSamples candidates from one Power_RIS tile (chosen by a stream shared by 256
// slots), streaming RIS against the cell's sphere (c, radius); the slot keeps the light and its contribution weight
// sum(w) / (p(sel) * BuildSamples), or is empty. The layouts differ only in the sphere.
PT_DEV uint2 di_regir_slot(const float4* __restrict__ lights, uint32_t count, const uint2* __restrict__ tiles, uint32_t g, v3 c, float radius,
                           uint32_t buildSamples, uint32_t frameIndex)
{
    uint32_t rng = ml_hash(rng_init(g & 0xFFFu, g >> 12, frameIndex) ^ kDIReGIRSalt);
    uint32_t coherent = ml_hash(rng_init(g >> 8, 0u, frameIndex) ^ kDIReGIRCoherentSalt);
    const uint2* tile = tiles + min((uint32_t)(rng_float(coherent) * (float)kDITileCount), kDITileCount - 1u) * kDITileSize;
    float wsum = 0.0f, pSel = 0.0f;
    uint32_t sel = ~0u;
    for (uint32_t k = 0; k < buildSamples; k++) {
        const float u = rng_float(rng), r = rng_float(rng);
        const uint2 e = tile[min((uint32_t)(u * (float)kDITileSize), kDITileSize - 1u)];
        const float p = e.x < count ? di_volume_weight(lights + kLightRec16 * (size_t)e.x, c, radius) : 0.0f;
        const float w = p > 0.0f ? p / (1.0f / __uint_as_float(e.y)) : 0.0f;      // target / source pdf
        wsum += w;
        if (r * wsum < w) { sel = e.x; pSel = p; }
    }
    return pSel > 0.0f ? make_uint2(sel, __float_as_uint(wsum / (pSel * (float)buildSamples))) : make_uint2(~0u, 0u);
}

// ReGIR build, Grid layout: one thread per slot; the cell's sphere is the cell centre and half its diagonal.
__global__ __launch_bounds__(256) void k_di_regir_build(const float4* __restrict__ lights, uint32_t count, const uint2* __restrict__ tiles, float cx0, float cy0, float cz0,
                                                        float cellSize, uint32_t buildSamples, uint32_t frameIndex, uint2* __restrict__ cells)
{
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= kDICellEntries) return;
    const uint32_t cell = g / kDICellLights;
    const uint32_t ix = cell % kDIGrid, iy = (cell / kDIGrid) % kDIGrid, iz = cell / (kDIGrid * kDIGrid);
    const float h = (float)(kDIGrid / 2u) - 0.5f;
    const v3 c = V3(cx0 + ((float)ix - h) * cellSize, cy0 + ((float)iy - h) * cellSize, cz0 + ((float)iz - h) * cellSize);
    const float radius = 0.5f * sqrtf(3.0f) * cellSize;
    cells[g] = di_regir_slot(lights, count, tiles, g, c, radius, buildSamples, frameIndex);
}

// ---- ReGIR Onion layout (pt_di_set_regir_layout; DESIGN.md section 1, "Local-light sampling") -----------------------------------------
// Cell 0 is the sphere of radius c = 0.5 * ReGIRCellSize around the camera; 15 layers follow, their boundaries growing by
// (p + pi) / (p - pi) per layer of a group with p partitions. A layer is cut into latitude rings of 2 pi / p (ring 0 the equatorial band,
// ring k >= 1 once per hemisphere, the last one a polar cap) and a ring into n cells of equal azimuth. The RTXDI SDK is not in the
// reference tree: the layout is this library's own after the SDK's structure, unpinned.
constexpr uint32_t kOnionGroups = 5u, kOnionLayers = 15u, kOnionCells = 2253u, kOnionRings = 20u, kOnionAzimuths = 241u;
constexpr uint32_t kDIOnionEntries = kOnionCells * kDICellLights;
static_assert(kDICellLights == 2u * 256u, "two blocks of the build per cell: the cell's sphere is uniform over a block");
static_assert(sizeof(PtDIReGIRLayoutSettings) == 16, "layout");
// Group g: p = 8 + 4 g partitions, g + 3 rings (g + 2 thresholds, the first of them at ring[g (g + 3) / 2]). The cells per ring are listed, so
// that no platform's cos decides a count; what follows from them is written out and checked where the tables are built.
constexpr uint32_t kOnionRingCells[kOnionGroups][7] = { { 8, 5, 1 }, { 12, 10, 6, 1 }, { 16, 14, 11, 6, 1 }, { 20, 19, 16, 11, 6, 1 }, { 24, 23, 20, 16, 12, 6, 1 } };
constexpr uint32_t onion_layer_base(uint32_t layer)            // the first cell of a layer: 20, 46, 80, 126 cells, then 180 per layer
{
    return layer >= 4u ? 273u + 180u * (layer - 4u) : layer == 0u ? 1u : layer == 1u ? 21u : layer == 2u ? 67u : 147u;
}
constexpr uint32_t onion_group_azimuth(uint32_t g) { return g == 0u ? 0u : g == 1u ? 11u : g == 2u ? 36u : g == 3u ? 79u : 146u; }   // a group's first azimuth threshold
struct OnionTables {
    float4 cells[kOnionCells];                      // unit scale: centre, radius of the bounding sphere
    float b2[16];                                   // squared layer boundaries, b2[0] = 1
    float ring[kOnionRings];                        // sin^2 of the rings' lower elevations, by group
    uint32_t ringStep[kOnionRings];                 // what passing ring[k] adds: cells before the ring | azimuth thresholds before it << 8 | the ring's cells << 16
    float azimuth[kOnionAzimuths + 3u];             // the pseudo-angles (di_diamond) between the cells of a ring, by (group, ring)
};
static_assert(sizeof(OnionTables) % 16 == 0 && kOnionRings % 4u == 0, "layout");
// monotone pseudo-angle of (x, z) around +y in [0, 4): one division instead of atan2
PT_DEV float di_diamond(float x, float z)
{
    if (z >= 0.0f) {
        if (x >= 0.0f) { const float s = x + z; return s > 0.0f ? z / s : 0.0f; }
        return 1.0f + (-x) / (z - x);
    }
    if (x < 0.0f) return 2.0f + (-z) / (-x - z);
    return 3.0f + x / (x - z);
}

// the cell of v (relative to the centre) at scale c; ~0u: beyond the last layer (or not a number). Every count is bounded by its
// table, so a cell index is < kOnionCells whatever v holds.
PT_DEV uint32_t di_onion_cell(const OnionTables* __restrict__ t, v3 v, float c)
{
    const float d2 = dot(v, v);
    const float q = d2 / (c * c);
    if (!(q < t->b2[15])) return ~0u;
    if (q < 1.0f) return 0u;
    // The layer and ring thresholds are read at uniform addresses, four to a trip: unrolled whole, their 36 SGPRs at once made the
    // temporal kernels spill. What a lane's ring selects -- the cells and azimuth thresholds before it, its own
    // cells -- is summed from ringStep as the group's thresholds pass: no per-lane address but the azimuths'.
    uint32_t layer = ~0u;                                                                     // b2[0] = 1 <= q < b2[15]
#pragma nounroll
    for (uint32_t l = 0; l < 16u; l += 4u)
#pragma unroll
        for (uint32_t i = 0; i < 4u; i++) layer += t->b2[l + i] <= q ? 1u : 0u;
    const uint32_t g = min(layer, kOnionGroups - 1u);
    uint32_t cell = onion_layer_base(layer);
    const float e = (v.y * v.y) / d2;
    uint32_t n = 8u + 4u * g, first = onion_group_azimuth(g);                                 // ring 0 of the group
    const uint32_t lo = g * (g + 3u) / 2u, cnt = g + 2u;                                      // the group's thresholds
    bool hemispheres = false;
#pragma nounroll
    for (uint32_t k = 0; k < kOnionRings; k += 4u) {
#pragma unroll
        for (uint32_t i = 0; i < 4u; i++) {                                                   // past a threshold: the next ring or beyond
            const bool in = k + i - lo < cnt && t->ring[k + i] <= e;
            const uint32_t step = t->ringStep[k + i];
            cell += in ? step & 0xFFu : 0u;
            first += in ? (step >> 8) & 0xFFu : 0u;
            n = in ? step >> 16 : n;
            hemispheres = hemispheres || in;
        }
    }
    cell += (hemispheres && v.y < 0.0f) ? n : 0u;                                             // ring k >= 1: north, then south
    const float A = di_diamond(v.x, v.z);
    for (uint32_t j = 0; j + 1u < n; j++) cell += t->azimuth[first + j] <= A ? 1u : 0u;       // per lane, at most 23
    return cell;
}

// ReGIR build, Onion layout: one thread per slot, two blocks per cell, so the cell's sphere is read through a uniform index.
__global__ __launch_bounds__(256) void k_di_regir_build_onion(const float4* __restrict__ lights, uint32_t count, const uint2* __restrict__ tiles,
                                                              const OnionTables* __restrict__ onion, float cx0, float cy0, float cz0, float c, uint32_t buildSamples,
                                                              uint32_t frameIndex, uint2* __restrict__ cells)
{
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= kDIOnionEntries) return;
    const float4 sph = onion->cells[blockIdx.x >> 1];
    cells[g] = di_regir_slot(lights, count, tiles, g, V3(cx0 + c * sph.x, cy0 + c * sph.y, cz0 + c * sph.z), c * sph.w, buildSamples, frameIndex);
}

// ---- initial sampling -------------------------------------------------------------------------------------------------------
// Candidate sources. begin(): the pixel's presampled entries (it may draw from the pixel's stream). pick(): a candidate's first draw r0 ->
// light li (false: an empty slot) and a value pv; pdf(pv, power, total): the light's source pdf, taken after the target, which reads the
// light's record and hands back its power.
struct DIEntries { const uint2* e; uint32_t n; };          // a Power_RIS tile or a ReGIR cell; none: no presampled entries

// the power CDF (PT_DI_LOCAL_LIGHT_POWER_CDF): select_light on the prefix sum, source pdf power / total
struct DIPowerCDF {
    PT_DEV DIEntries begin(const DIArgs&, const DISurface&, uint32_t, uint32_t, uint32_t&) const { return DIEntries{ nullptr, 0u }; }
    PT_DEV bool pick(const DIArgs& a, DIEntries, float r0, float total, uint32_t& li, float&) const { li = select_light(a.cdf, a.count, r0 * total, total); return true; }
    PT_DEV float pdf(float, float power, float total) const { return power / total; }
    PT_DEV float light_pdf(const DIArgs&, float power, float total) const { return power / total; }     // of a light no draw of the source produced
};

// Uniform, Power_RIS or ReGIR (the mode is uniform over the grid). Power_RIS: the pixel's screen tile picks a light tile. ReGIR: three
// jitter draws from the pixel stream pick the cell (of the Grid or the Onion layout, uniform over the grid too); outside the cells,
// Power_RIS. Uniform: 1 / count; an entry: 1 / its inverse pdf.
struct DISampling {
    uint32_t mode; const uint2* tiles; const uint2* cells; float centre[3], cellSize;
    uint32_t layout; const OnionTables* onion;          // PT_DI_REGIR_LAYOUT_*; the tables under ONION
    PT_DEV DIEntries begin(const DIArgs& a, const DISurface& s, uint32_t x, uint32_t y, uint32_t& rng) const
    {
        DIEntries src{ nullptr, 0u };
        if (mode != PT_DI_LOCAL_LIGHT_UNIFORM) {
            uint32_t ts = ml_hash(rng_init(x / kDIScreenTile, y / kDIScreenTile, a.frameIndex) ^ kDIScreenTileSalt);
            src.e = tiles + min((uint32_t)(rng_float(ts) * (float)kDITileCount), kDITileCount - 1u) * kDITileSize;
            src.n = kDITileSize;
        }
        if (mode == PT_DI_LOCAL_LIGHT_REGIR_RIS) {
            const float jx = (rng_float(rng) - 0.5f) * kDIJitterScale, jy = (rng_float(rng) - 0.5f) * kDIJitterScale, jz = (rng_float(rng) - 0.5f) * kDIJitterScale;
            uint32_t cell = ~0u;
            if (layout == PT_DI_REGIR_LAYOUT_ONION) {                     // the jitter grows with the distance, as the cells do (pi / 12)
                const float c = 0.5f * cellSize;                           // RTXDI.ixx:92
                const v3 v0 = V3(s.P.x - centre[0], s.P.y - centre[1], s.P.z - centre[2]);
                const float sc = fmaxf(c, 0.2617994f * sqrtf(dot(v0, v0)));
                cell = di_onion_cell(onion, V3(v0.x + jx * sc, v0.y + jy * sc, v0.z + jz * sc), c);
            } else {
                const float fx = floorf((s.P.x + jx * cellSize - centre[0]) / cellSize), fy = floorf((s.P.y + jy * cellSize - centre[1]) / cellSize),
                            fz = floorf((s.P.z + jz * cellSize - centre[2]) / cellSize);
                const float lim = (float)(kDIGrid / 2u);
                if (fx >= -lim && fx < lim && fy >= -lim && fy < lim && fz >= -lim && fz < lim)
                    cell = (((uint32_t)((int)fz + (int)(kDIGrid / 2u)) * kDIGrid) + (uint32_t)((int)fy + (int)(kDIGrid / 2u))) * kDIGrid + (uint32_t)((int)fx + (int)(kDIGrid / 2u));
            }
            if (cell != ~0u) {
                src.e = cells + (size_t)cell * kDICellLights;
                src.n = kDICellLights;
            }
        }
        return src;
    }
    PT_DEV bool pick(const DIArgs& a, DIEntries src, float r0, float, uint32_t& li, float& pdf) const
    {
        if (src.e) {
            const uint2 e = src.e[min((uint32_t)(r0 * (float)src.n), src.n - 1u)];
            li = e.x; pdf = 1.0f / __uint_as_float(e.y);
        } else {
            li = min((uint32_t)(r0 * (float)a.count), a.count - 1u); pdf = 1.0f / (float)a.count;
        }
        return li < a.count;
    }
    PT_DEV float pdf(float pv, float, float) const { return pv; }
    // RAB_EvaluateLocalLightSourcePdf of a light that came out of no tile or cell: Uniform 1 / count, else power / total (with the PDF texture
    // acting, a.total holds top * M * M in place of the prefix sum's total)
    PT_DEV float light_pdf(const DIArgs& a, float power, float total) const { return mode == PT_DI_LOCAL_LIGHT_UNIFORM ? 1.0f / (float)a.count : power / total; }
};

// LocalLightSamples candidates from a source, streaming RIS (RTXDI_StreamSample); the selected sample's shaded terms stay in registers
struct DIInitial { float wsum, p; v3 dif, spc, pos; float u, v; uint32_t li; };

// ---- BRDF candidates (pt_di_set_brdf_sampling; DESIGN.md section 1, "BRDF candidates") -------------------------------------------------
constexpr uint32_t kDIBrdfSalt = 0x44490008u;        // the BRDF candidates' stream: five draws per candidate, r0..r3 (Sample), r4 (the RIS coin)
static_assert(sizeof(uint4) == 4u * PT_DI_BRDF_CANDIDATE_WORDS, "layout");
// candidates of a pixel, the reservoir's M: light samples plus, in the BRDF instantiations, BRDF samples
template <bool BRDF> PT_DEV uint32_t di_candidates(const DIArgs& a) { if constexpr (BRDF) return a.samples + a.brdfSamples; else return a.samples; }
// how far a BRDF ray of pdf q reaches under BrdfCutoff c > 0
PT_DEV float di_brdf_range(float cutoff, float q) { return sqrtf((1.0f / cutoff - 1.0f) * q); }
// the pdf a sample of light-source pdf qL is weighted against with both techniques on: (N_L qL + N_B qB / pdfSA) / N, the BRDF pdf
// counting as 0 beyond the cutoff range. (Never taken with N_B = 0: (N_L x) / N_L is not x.)
PT_DEV float di_blended_pdf(const DIArgs& a, float qL, const DIMisTerms& m)
{
    const float nl = (float)a.samples, nb = (float)a.brdfSamples, n = (float)(a.samples + a.brdfSamples);
    if (!(m.pdfSA > 0.0f) || !isfinite(m.pdfSA)) return nl * qL / n;
    float qB = m.pdfBrdf;
    if (a.brdfCutoff > 0.0f && m.dist > di_brdf_range(a.brdfCutoff, qB)) qB = 0.0f;
    return (nl * qL + nb * qB / m.pdfSA) / n;
}

// BRDF = true: the RIS weight of a light candidate is target / blended pdf, and the pixel's BRDF records follow the light candidates into
// the same reservoir, each a light sample (li, U, V) of source pdf light_pdf with the stream's fifth draw as its coin.
template <bool BRDF = false, typename Source>
PT_DEV void di_initial(const DIArgs& a, const Source& source, const DISurface& s, uint32_t x, uint32_t y, size_t pi, float total, DIInitial& o)
{
    uint32_t rng = ml_hash(rng_init(x, y, a.frameIndex) ^ kDISalt);
    o.wsum = 0.0f; o.p = 0.0f; o.u = 0.0f; o.v = 0.0f; o.li = ~0u;
    o.dif = V3(0, 0, 0); o.spc = V3(0, 0, 0); o.pos = V3(0, 0, 0);
    const DIEntries src = source.begin(a, s, x, y, rng);
    for (uint32_t k = 0; k < a.samples; k++) {
        const float r0 = rng_float(rng), r1 = rng_float(rng), r2 = rng_float(rng), r3 = rng_float(rng);
        uint32_t li;
        float pv;
        const bool some = source.pick(a, src, r0, total, li, pv);
        v3 pos = V3(0, 0, 0), dif = V3(0, 0, 0), spc = V3(0, 0, 0);
        float power = 0.0f;
        DIMisTerms mis;
        const float p = some ? di_target(a, s, li, r1, r2, pos, dif, spc, power, BRDF ? &mis : nullptr) : 0.0f;    // an empty slot: weight 0, still counted in M
        float ris;
        if constexpr (BRDF) ris = p > 0.0f ? p / di_blended_pdf(a, source.pdf(pv, power, total), mis) : 0.0f;
        else ris = p > 0.0f ? p / source.pdf(pv, power, total) : 0.0f;  // target / source pdf (light selection; the point is uniform in uv)
        o.wsum += ris;
        if (r3 * o.wsum < ris) { o.p = p; o.dif = dif; o.spc = spc; o.pos = pos; o.u = r1; o.v = r2; o.li = li; }
    }
    if constexpr (BRDF) {
        uint32_t brng = ml_hash(rng_init(x, y, a.frameIndex) ^ kDIBrdfSalt);
        for (uint32_t j = 0; j < a.brdfSamples; j++) {
            rng_float(brng); rng_float(brng); rng_float(brng); rng_float(brng);
            const float r4 = rng_float(brng);
            const uint4 rec = a.brdfRecords[pi * a.brdfSamples + j];
            if (rec.x >= a.count) continue;                                 // no light at the end of the ray: weight 0, counted in M
            const float U = __uint_as_float(rec.y), V = __uint_as_float(rec.z);
            v3 pos = V3(0, 0, 0), dif = V3(0, 0, 0), spc = V3(0, 0, 0);
            float power = 0.0f;
            DIMisTerms mis;
            const float p = di_target(a, s, rec.x, U, V, pos, dif, spc, power, &mis);
            const float ris = p > 0.0f ? p / di_blended_pdf(a, source.light_pdf(a, power, total), mis) : 0.0f;
            o.wsum += ris;
            if (r4 * o.wsum < ris) { o.p = p; o.dif = dif; o.spc = spc; o.pos = pos; o.u = U; o.v = V; o.li = rec.x; }
        }
    }
}
// W of the initial reservoir: (sum w / M) / target(y); with BRDF candidates sum w / (M target(y))
template <bool BRDF> PT_DEV float di_initial_weight(const DIArgs& a, const DIInitial& i0)
{
    if constexpr (BRDF) return i0.wsum / ((float)(a.samples + a.brdfSamples) * i0.p);
    else return i0.wsum / (float)a.samples / i0.p;
}

// the visibility ray every DI pass traces (CreateVisibilityRay with offset 1e-3): from P to pos, tmin 1e-3, tmax = max(0, dist - 2e-3).
// vis: the coloured visibility; returns whether the any-hit walk committed something (GetConservativeVisibility: blocked)
PT_DEV bool di_shadow_ray(BlobView bv, const AlphaContext& ac, DeviceCounters* counters, uint2* ldsStack, v3 P, v3 pos, float& dist, v3& vis)
{
    const v3 d = pos - P;
    dist = sqrtf(dot(d, d));
    const v3 dir = V3(d.x / dist, d.y / dist, d.z / dist);
    uint2 spill[kStackSize - kLdsStackDepth];
    GroupStack<kLdsStackDepth> stack; stack.init((PT_LDS_AS void*)ldsStack, spill);
    BlobReader<false> blob; blob.p = bv.base;
    TraceStats st; st.nodes = 0; st.tris = 0; st.overflow = 0;
    const Hit h = trace_single<false, false, true>(blob, bv, ac, P, dir, 1e-3f, fmaxf(0.0f, dist - 2e-3f), stack, &st, &vis);
    if (st.overflow) atomicAdd(&counters->stackOverflows, st.overflow);
    return h.inst != ~0u;
}

// the outputs of final shading (DIFinalShading.hlsl:78-103) for a sample of visibility vis at distance dist
PT_DEV void di_final_write(const DIArgs& a, size_t pi, float dist, v3 vis, v3 difSel, v3 spcSel, float W)
{
    const PtTextures& tx = a.tx;
    if (vis.x == 0.0f && vis.y == 0.0f && vis.z == 0.0f) return;
    const v3 dif = V3(difSel.x * vis.x * W, difSel.y * vis.y * W, difSel.z * vis.z * W);
    const v3 spc = V3(spcSel.x * vis.x * W, spcSel.y * vis.y * W, spcSel.z * vis.z * W);
    const v3 rad = dif + spc;
    if ((rad.x == 0.0f && rad.y == 0.0f && rad.z == 0.0f) || !finite3(rad)) return;

    if (a.lastPass && a.denoiser <= PT_DENOISER_DLSS_RAY_RECONSTRUCTION) {
        ushort4* R = (ushort4*)tx.Radiance;
        const ushort4 o = R[pi];
        const v3 sum = V3(f16_to_f32(o.x) + rad.x, f16_to_f32(o.y) + rad.y, f16_to_f32(o.z) + rad.z);
        R[pi] = make_ushort4(f32_to_f16(sum.x), f32_to_f16(sum.y), f32_to_f16(sum.z), o.w);
        if (tx.RadianceF32) ((float4*)tx.RadianceF32)[pi] = make_float4(sum.x, sum.y, sum.z, 0.0f);
        if (a.denoiser == PT_DENOISER_DLSS_RAY_RECONSTRUCTION && tx.SpecularHitDistance && (spc.x > 0.0f || spc.y > 0.0f || spc.z > 0.0f))
            ((uint16_t*)tx.SpecularHitDistance)[pi] = f32_to_f16(dist);
        return;
    }
    ((ushort4*)tx.Diffuse)[pi] = make_ushort4(f32_to_f16(dif.x), f32_to_f16(dif.y), f32_to_f16(dif.z), f32_to_f16(dist));
    ((ushort4*)tx.Specular)[pi] = make_ushort4(f32_to_f16(spc.x), f32_to_f16(spc.y), f32_to_f16(spc.z), f32_to_f16(dist));
}

// The pixel of a thread (x, local row): a wave covers an 8 x 8 square of the block's 16 x 16 (as k_gbuffer), so the rays of a wave stay together.
PT_DEV void di_pixel(uint32_t& x, uint32_t& ly)
{
    const uint32_t wv = threadIdx.x >> 6, ln = threadIdx.x & 63u;
    x = blockIdx.x * 16 + (wv & 1u) * 8u + (ln & 7u); ly = blockIdx.y * 16 + (wv >> 1) * 8u + (ln >> 3);
}

// The plain pass, no reuse: initial sampling from a candidate source, then final shading. One thread per local pixel.
template <typename Source, bool BRDF = false>
__global__ __launch_bounds__(256) void k_di(DIArgs a, Source source, BlobView bv, AlphaContext ac, DeviceCounters* counters)
{
    uint32_t x, ly; di_pixel(x, ly);
    if (x >= a.fv.width || ly >= a.fv.localRows) return;                 // no barrier below
    const uint32_t y = global_row(a.fv, ly);
    const size_t pi = (size_t)ly * a.fv.width + x;
    DISurface s;
    if (!di_surface(a, a.view, pi, x, y, s)) return;
    const float total = *a.total;
    if (!(total > 0.0f) || !isfinite(total)) return;
    DIInitial i0;
    di_initial<BRDF>(a, source, s, x, y, pi, total, i0);
    if (!(i0.p > 0.0f)) return;
    __shared__ uint2 ldsStack[kLdsStackDepth * 256];
    float dist; v3 vis;
    di_shadow_ray(bv, ac, counters, ldsStack, s.P, i0.pos, dist, vis);
    di_final_write(a, pi, dist, vis, i0.dif, i0.spc, di_initial_weight<BRDF>(a, i0));   // W = (sum w / M) / target(y)
}

// The BRDF candidates' rays, ahead of initial sampling: one thread per local pixel, a wave on an 8 x 8 square. Per candidate the five draws
// of the stream, an all-lobe Sample as RAB_Surface::Sample takes it, the all-lobe pdf of the direction, and -- when there is a direction of
// positive pdf -- one closest-hit walk (the renderer's rule: alpha test on non-opaque geometry) from (P, 1e-3) out to the cutoff range.
// A hit on an emissive object becomes the light sample (first[object] + primitive, U, V) that Math::SampleTriangle maps back to the hit point:
// with hit barycentrics (b1, b2), sqrt(U) = b1 + b2 and V = b2 / (b1 + b2). Every local pixel writes its records, the empty surface empty ones.
// The walk's stack is di_shadow_ray's: kLdsStackDepth entries per lane in LDS, the rest spilled, overflows counted.
__global__ __launch_bounds__(256) void k_di_brdf_rays(DIArgs a, uint4* __restrict__ records, BlobView bv, AlphaContext ac, DeviceCounters* counters)
{
    uint32_t x, ly; di_pixel(x, ly);
    if (x >= a.fv.width || ly >= a.fv.localRows) return;                 // no barrier below
    const uint32_t y = global_row(a.fv, ly);
    const size_t pi = (size_t)ly * a.fv.width + x;
    DISurface s;
    const bool valid = di_surface(a, a.view, pi, x, y, s);
    __shared__ uint2 ldsStack[kLdsStackDepth * 256];
    uint2 spill[kStackSize - kLdsStackDepth];
    GroupStack<kLdsStackDepth> stack; stack.init((PT_LDS_AS void*)ldsStack, spill);
    BlobReader<false> blob; blob.p = bv.base;
    TraceStats st; st.nodes = 0; st.tris = 0; st.overflow = 0;
    uint32_t rng = ml_hash(rng_init(x, y, a.frameIndex) ^ kDIBrdfSalt);
    for (uint32_t j = 0; j < a.brdfSamples; j++) {
        float rnd[4];
        rnd[0] = rng_float(rng); rnd[1] = rng_float(rng); rnd[2] = rng_float(rng); rnd[3] = rng_float(rng);   // GetFloat4
        rng_float(rng);                                                   // r4: the coin, di_initial's
        uint4 rec = make_uint4(~0u, 0u, 0u, 0u);
        v3 L = V3(0.0f, 0.0f, 0.0f); int lobe = 0;
        if (valid && s.bs.Sample(s.svec, s.V, s.w, rnd, L, lobe)) {
            float q; v3 dif, spc;
            s.bs.EvaluateAll(s.svec, L, s.V, s.w, q, dif, spc, a.ext);
            if (q > 0.0f) {
                rec.w = __float_as_uint(q);
                const float tmax = a.brdfCutoff > 0.0f ? di_brdf_range(a.brdfCutoff, q) : 3.402823466e+38f;
                const Hit h = trace_single<false, false, false>(blob, bv, ac, s.P, L, 1e-3f, tmax, stack, &st, nullptr);
                if (h.inst != ~0u) {
                    const uint32_t object = ac.instances[h.inst].instanceID + h.geom;
                    const uint32_t first = object < a.objectCount ? a.firstLight[object] : ~0u;
                    if (first != ~0u) {
                        const float t = h.u + h.v;
                        rec.x = first + h.prim;
                        if (t != 0.0f) { rec.y = __float_as_uint(t * t); rec.z = __float_as_uint(h.v / t); }
                    }
                }
            }
        }
        records[pi * a.brdfSamples + j] = rec;
    }
    if (st.overflow) atomicAdd(&counters->stackOverflows, st.overflow);
}

// ---- reservoir reuse (DITemporalResampling / DISpatialResampling; DESIGN.md section 1, "Reservoir reuse") --------------------------------
constexpr uint32_t kDITemporalSalt = 0x44490002u, kDISpatialSalt = 0x44490003u;
constexpr uint32_t kDIOffsetCount = 8192u;          // neighbour-offset table entries (int8 x, y)
static_assert(sizeof(PtDIReservoir) == 32 && sizeof(PtDIResamplingSettings) == 64 && sizeof(PtDIPreviousTextures) == 48 && sizeof(PtDIVisibilitySettings) == 32, "layout");
static_assert(sizeof(PtDIPairwiseSettings) == 16, "layout");
// BIAS of the reuse kernels, the normalisation of a pass: Off (1 / M), Basic, or Pairwise (BASIC + pt_di_set_pairwise's flag)
constexpr uint32_t kDIBiasOff = 0u, kDIBiasBasic = 1u, kDIBiasPairwise = 2u;

struct DIReuseArgs {
    DIArgs d;
    DIView prev;                                    // the previous frame's G-buffer and camera (temporal reuse)
    const PtDIReservoir* in; PtDIReservoir* out;  // temporal: last frame's final reservoirs -> A; spatial: A -> B
    const char2* offsets;
    uint32_t haveHistory, maxHistory, boiling, spatialSamples, boostSamples;
    float boilingMul, tDepth, tNormal, radius, sDepth, sNormal;
};

PT_DEV PtDIReservoir di_empty(uint32_t M)
{
    PtDIReservoir r; r.LightIndex = ~0u; r.U = 0.0f; r.V = 0.0f; r.W = 0.0f; r.M = M; r.TargetPdf = 0.0f; r.Age = 0u; r.Visibility = 0u;
    return r;
}
// VIS: the reservoirs carry the Visibility word (pt_di_set_visibility); without it the word is read and written as 0
template <bool VIS = false>
PT_DEV PtDIReservoir di_load(const PtDIReservoir* p, size_t i)
{
    const uint4 a = ((const uint4*)p)[2 * i], b = ((const uint4*)p)[2 * i + 1];
    PtDIReservoir r; r.LightIndex = a.x; r.U = __uint_as_float(a.y); r.V = __uint_as_float(a.z); r.W = __uint_as_float(a.w);
    r.M = b.x; r.TargetPdf = __uint_as_float(b.y); r.Age = b.z; r.Visibility = VIS ? b.w : 0u;
    return r;
}
template <bool VIS = false>
PT_DEV void di_store(PtDIReservoir* p, size_t i, const PtDIReservoir& r)
{
    ((uint4*)p)[2 * i] = make_uint4(r.LightIndex, __float_as_uint(r.U), __float_as_uint(r.V), __float_as_uint(r.W));
    ((uint4*)p)[2 * i + 1] = make_uint4(r.M, __float_as_uint(r.TargetPdf), r.Age, VIS ? r.Visibility : 0u);
}

// ---- reservoir visibility (pt_di_set_visibility; DESIGN.md section 1, "Reservoir visibility") ------------------------------------------
// What the visibility-enabled instantiations take on top of DIReuseArgs: the traversal's inputs and the settings.
struct DIVisArgs {
    BlobView bv; AlphaContext ac; DeviceCounters* counters;
    uint32_t initial, maxAge, discard;              // maxAge 0: no final-visibility reuse
    float maxDistance;
};
// VIS of the reuse kernels: 0 off; kDIVisOn: the reservoirs carry the Visibility word; | kDIVisRaytraced: Basic bias correction traces
constexpr uint32_t kDIVisOn = 1u, kDIVisRaytraced = 2u;
// The settings reach the visibility-enabled instantiations as one trailing DIVisArgs; without VIS a kernel's arguments end before it.
PT_DEV const DIVisArgs* di_vis_args() { return nullptr; }
PT_DEV const DIVisArgs* di_vis_args(const DIVisArgs& va) { return &va; }
// PtDIReservoir.Visibility: rgb 5 bits each | dx, dy 6-bit two's complement clamped to +-31 | age 4 bits saturating
PT_DEV uint32_t di_vis_pack(v3 vis)
{
    const uint32_t r = (uint32_t)(fminf(fmaxf(vis.x, 0.0f), 1.0f) * 31.0f), g = (uint32_t)(fminf(fmaxf(vis.y, 0.0f), 1.0f) * 31.0f),
                   b = (uint32_t)(fminf(fmaxf(vis.z, 0.0f), 1.0f) * 31.0f);
    return r | (g << 5) | (b << 10);
}
PT_DEV v3 di_vis_colour(uint32_t w) { return V3((float)(w & 31u) / 31.0f, (float)((w >> 5) & 31u) / 31.0f, (float)((w >> 10) & 31u) / 31.0f); }
PT_DEV int di_vis_delta(uint32_t w, uint32_t shift) { return (int)((w >> shift) & 63u) - (int)((w >> shift) & 32u) * 2; }
// the word of a sample taken from pixel (x + ddx, y + ddy), dAge frames later
PT_DEV uint32_t di_vis_carry(uint32_t w, int ddx, int ddy, uint32_t dAge)
{
    const int dx = min(max(di_vis_delta(w, 15u) + ddx, -31), 31), dy = min(max(di_vis_delta(w, 21u) + ddy, -31), 31);
    const uint32_t age = min(((w >> 27) & 15u) + dAge, 15u);
    return (w & 0x7FFFu) | (((uint32_t)dx & 63u) << 15) | (((uint32_t)dy & 63u) << 21) | (age << 27);
}
// final shading may use the stored visibility: 1 <= age <= maxAge and |d| < maxDistance (a d clamped to 31 never is: maxDistance <= 31)
PT_DEV bool di_vis_reusable(uint32_t w, uint32_t maxAge, float maxDistance)
{
    const uint32_t age = (w >> 27) & 15u;
    const int dx = di_vis_delta(w, 15u), dy = di_vis_delta(w, 21u);
    return age >= 1u && age <= maxAge && sqrtf((float)(dx * dx + dy * dy)) < maxDistance;
}
// the point of sample (li, U, V): the arithmetic of di_target
PT_DEV v3 di_sample_point(const DIArgs& a, uint32_t li, float U, float V)
{
    const float4* L = a.lights + kLightRec16 * (size_t)li;
    const float4 l0 = L[0], l1 = L[1], l2 = L[2];
    const float sq = sqrtf(U);
    const float b0 = sq * (1.0f - V), b1 = sq * V;
    return V3(l0.x + l1.x * b0 + l2.x * b1, l0.y + l1.y * b0 + l2.y * b1, l0.z + l1.z * b0 + l2.z * b1);
}
// RAB_ClampSamplePositionIntoView: reflect across the screen edges (one reflection; a position still outside reads the empty surface)
PT_DEV void di_reflect(int& x, int& y, int w, int h)
{
    if (x < 0) x = -x;
    if (y < 0) y = -y;
    if (x >= w) x = 2 * w - x - 1;
    if (y >= h) y = 2 * h - y - 1;
}
// spatial sample i's neighbour (qx, qy) of pixel (x, y): offset-table entry start + i scaled by the radius, reflected; false: outside the view
PT_DEV bool di_neighbour(const DIReuseArgs& r, uint32_t x, uint32_t y, uint32_t start, uint32_t i, int& qx, int& qy)
{
    const int w = (int)r.d.fv.width, h = (int)r.d.fv.height;
    const char2 e = r.offsets[(start + i) & (kDIOffsetCount - 1u)];
    qx = (int)x + (int)((float)e.x / 127.0f * r.radius); qy = (int)y + (int)((float)e.y / 127.0f * r.radius);
    di_reflect(qx, qy, w, h);
    return qx >= 0 && qy >= 0 && qx < w && qy < h;
}
// the neighbour test: shading normals, relative depth (RTXDI_CompareRelativeDifference) and RAB_AreMaterialsSimilar
PT_DEV bool di_similar(const DISurface& a, const DISurface& b, float depthA, float normalThreshold, float depthThreshold)
{
    if (!(dot(a.svec.ShadingNormal, b.svec.ShadingNormal) >= normalThreshold)) return false;
    if (!(fabsf(depthA - b.depth) <= depthThreshold * fmaxf(depthA, b.depth))) return false;
    if (!(fabsf(a.bs.Roughness - b.bs.Roughness) <= 0.5f * fmaxf(a.bs.Roughness, b.bs.Roughness))) return false;
    return fabsf(ml_luminance(a.bs.F0) - ml_luminance(b.bs.F0)) <= 0.25f && fabsf(ml_luminance(a.bs.Albedo) - ml_luminance(b.bs.Albedo)) <= 0.25f;
}
PT_DEV float di_target_of(const DIArgs& a, const DISurface& s, uint32_t li, float U, float V)
{
    if (li >= a.count) return 0.0f;
    v3 pos, dif, spc;
    float power;
    return di_target(a, s, li, U, V, pos, dif, spc, power);
}

// ---- pairwise MIS (pt_di_set_pairwise; DESIGN.md section 1, "Pairwise bias correction") ----------------------------------------------
// One pair (canonical c, neighbour i) of n attempted slots at a sample y: a = (n * M_i) * p_i(y), b = M_c * p_c(y), D = a + b. The
// neighbour's share of y is a / D and the canonical's b / D; D = 0 gives 0. The caller scales by 1 / (n + 1).
PT_DEV float di_pair_share(float mine, float other)
{
    const float D = mine + other;
    return D > 0.0f ? mine / D : 0.0f;
}

// the temporal pass's history search: the motion-vector position, then eight jittered ones (draws from the temporal stream); returns the
// pixel index in the w x h previous frame of the first whose previous surface sp passes the neighbour test against the expected depth, or -1.
// The position comes back in one int: as two by-reference outputs it cost the Basic instantiations a wave per SIMD.
PT_DEV int di_find_history(const DIReuseArgs& r, const DISurface& s, int w, int h, uint32_t x, uint32_t y, size_t pi, uint32_t& rng, DISurface& sp)
{
    const DIArgs& a = r.d;
    const ushort4 mv = ((const ushort4*)a.tx.MotionVector)[pi];
    const float expected = s.depth + f16_to_f32(mv.z);
    const float fx = fminf(fmaxf((float)x + f16_to_f32(mv.x), -65536.0f), 65536.0f), fy = fminf(fmaxf((float)y + f16_to_f32(mv.y), -65536.0f), 65536.0f);
    const int px = (int)rintf(fx), py = (int)rintf(fy);            // HLSL round: to nearest even
    for (int i = 0; i < 9; i++) {
        int qx = px, qy = py;
        if (i) { const float rx = rng_float(rng), ry = rng_float(rng); qx += (int)((rx - 0.5f) * 6.0f); qy += (int)((ry - 0.5f) * 6.0f); }
        di_reflect(qx, qy, w, h);
        if (qx < 0 || qy < 0 || qx >= w || qy >= h) continue;
        if (!di_surface(a, r.prev, (size_t)qy * w + qx, qx, qy, sp)) continue;
        if (!di_similar(s, sp, expected, r.tNormal, r.tDepth)) continue;
        return qy * w + qx;
    }
    return -1;
}
// boiling filter: the tile's mean of the nonzero weights, a 64-lane butterfly (every lane of the wave takes part)
PT_DEV void di_boiling(const DIReuseArgs& r, bool valid, PtDIReservoir& res)
{
    const bool nz = valid && res.W > 0.0f;
    float sum = nz ? res.W : 0.0f, cnt = nz ? 1.0f : 0.0f;
    for (int m = 1; m < 64; m <<= 1) { sum += __shfl_xor(sum, m); cnt += __shfl_xor(cnt, m); }
    if (cnt > 0.0f && res.W > sum / cnt * r.boilingMul) res = di_empty(0u);
}

// Initial sampling from a candidate source fused with temporal reuse: the temporal step at a pixel reads only that pixel's fresh reservoir
// and last frame's data. TEMPORAL = false writes the initial reservoirs (the spatial pass's input). The boiling filter is a 64-lane
// butterfly over the wave's 8 x 8 tile, so every lane stays to the end.
// VIS != 0 (pt_di_set_visibility, encoded as above): initial visibility traces the selected initial sample's ray, and blocked empties the
// reservoir; a selected history sample brings its Visibility word along, moved by the pixel offset and one frame older. kDIVisRaytraced
// (with BASIC): p at the previous surface counts as 0 when the ray from the current surface to the selected sample is blocked. The two
// rays of a lane depend on each other (the second sample is chosen after the first ray), so they are the two trips of one loop that all
// lanes walk together: lanes without a ray on a trip trace nothing, and every lane reaches the boiling filter's butterfly. The loop is
// unrolled, i.e. two inlined walks: kept rolled around one trace site the kernel needs 185 VGPRs (2 waves per SIMD), unrolled 137
// (3 waves), scratch 464 B / lane either way. Without VIS there is no loop, no ray and no group stack in LDS.
// BIAS = kDIBiasPairwise: the fresh reservoir is the canonical domain and the history the one neighbour (n = 1); p at the previous surface
// is taken for both samples, the weights and W come from the temporal step itself and nothing waits for a ray.
template <bool TEMPORAL, uint32_t BIAS, uint32_t VIS, bool BRDF, typename Source, typename... Extra>
__global__ __launch_bounds__(256) void k_di_initial_temporal(DIReuseArgs r, Source source, Extra... extra)
{
    constexpr bool BASIC = BIAS == kDIBiasBasic, PAIRWISE = BIAS == kDIBiasPairwise;
    constexpr bool CARRY = VIS != 0u, RAYTRACED = (VIS & kDIVisRaytraced) != 0u;
    static_assert(!PAIRWISE || TEMPORAL, "a normalisation belongs to a pass that is on");
    static_assert(!RAYTRACED || (TEMPORAL && BASIC), "the raytraced normalisation is Basic bias correction's");
    const DIArgs& a = r.d;
    uint32_t x, y; di_pixel(x, y);
    const bool inside = x < a.fv.width && y < a.fv.localRows;             // unsharded: local row = global row
    const size_t pi = (size_t)y * a.fv.width + x;
    PtDIReservoir res = di_empty(0u);
    DISurface s;
    const bool valid = inside && di_surface(a, a.view, pi, x, y, s);
    v3 target = V3(0.0f, 0.0f, 0.0f);                                      // where this trip's ray goes
    bool want = false;
    uint32_t Mcur = 0, MH = 0;                                            // Basic's normalisation waits for the second ray
    float wsum = 0.0f, pPrev = 0.0f;
    bool fromH = false, basicPending = false;
    // the temporal step of a valid pixel. Without VIS it runs inside the block of the initial sampling: behind the block, as with VIS, it
    // took three of those instantiations one VGPR more
    auto temporal = [&]() {
        const int w = (int)a.fv.width, h = (int)a.fv.height;
        uint32_t rng = ml_hash(rng_init(x, y, a.frameIndex) ^ kDITemporalSalt);
        DISurface sp;
        const int hi = r.haveHistory ? di_find_history(r, s, w, h, x, y, pi, rng, sp) : -1;
        // combine(s, R0, 0.5, p(y0)) selects R0; then combine(s, H, rc, p(yH)) with the draw after every search draw
        Mcur = res.M;
        if constexpr (PAIRWISE) {                                       // no history pixel: the fresh reservoir as it is. (The return below
                                                                        // leaves this lambda; the lane goes on to the boiling filter.)
            if (hi >= 0) {
                PtDIReservoir H = di_load<CARRY>(r.in, (size_t)hi);
                H.M = min(H.M, r.maxHistory * Mcur);
                const float pH = di_target_of(a, s, H.LightIndex, H.U, H.V);
                const float rc = rng_float(rng);
                const float pc = res.TargetPdf;
                const float mH = di_pair_share((float)H.M * di_target_of(a, sp, H.LightIndex, H.U, H.V), (float)Mcur * pH) * 0.5f;    // n = 1
                const float mc = (1.0f + di_pair_share((float)Mcur * pc, (float)H.M * di_target_of(a, sp, res.LightIndex, res.U, res.V))) * 0.5f;
                const float wH = mH * pH * H.W;
                wsum = mc * pc * res.W + wH;
                if (rc * wsum < wH) {
                    res.LightIndex = H.LightIndex; res.U = H.U; res.V = H.V; res.TargetPdf = pH; res.Age = H.Age == ~0u ? ~0u : H.Age + 1u;
                    if constexpr (CARRY) res.Visibility = di_vis_carry(H.Visibility, hi % w - (int)x, hi / w - (int)y, 1u);
                }
                res.M = Mcur + H.M;
                if (res.TargetPdf > 0.0f) res.W = wsum / res.TargetPdf; else res = di_empty(res.M);
            }
            return;
        }
        wsum = res.TargetPdf * res.W * (float)res.M;
        if (hi >= 0) {
            PtDIReservoir H = di_load<CARRY>(r.in, (size_t)hi);
            H.M = min(H.M, r.maxHistory * Mcur);
            const float pH = di_target_of(a, s, H.LightIndex, H.U, H.V);
            const float rc = rng_float(rng);
            const float wH = pH * H.W * (float)H.M;
            wsum += wH;
            if (rc * wsum < wH) {
                res.LightIndex = H.LightIndex; res.U = H.U; res.V = H.V; res.TargetPdf = pH; res.Age = H.Age == ~0u ? ~0u : H.Age + 1u; fromH = true;
                if constexpr (CARRY) res.Visibility = di_vis_carry(H.Visibility, hi % w - (int)x, hi / w - (int)y, 1u);
            }
            MH = H.M;
            res.M = Mcur + H.M;
        }
        const float p = res.TargetPdf;
        if (!(p > 0.0f)) {
            res = di_empty(res.M);
        } else if (BASIC) {                                             // p at the previous surface: no visibility but RAYTRACED's
            pPrev = hi >= 0 ? di_target_of(a, sp, res.LightIndex, res.U, res.V) : 0.0f;
            basicPending = true;
            if (RAYTRACED && hi >= 0 && pPrev > 0.0f) { want = true; target = di_sample_point(a, res.LightIndex, res.U, res.V); }
        } else {
            res.W = wsum / (p * (float)res.M);
        }
    };
    if (valid) {
        res.M = di_candidates<BRDF>(a);
        const float total = *a.total;
        if (total > 0.0f && isfinite(total)) {
            DIInitial i0;
            di_initial<BRDF>(a, source, s, x, y, pi, total, i0);
            if (i0.p > 0.0f) {
                res.LightIndex = i0.li; res.U = i0.u; res.V = i0.v; res.W = di_initial_weight<BRDF>(a, i0); res.TargetPdf = i0.p;
                if constexpr (CARRY) { target = i0.pos; want = di_vis_args(extra...)->initial != 0u; }
            }
        }
        if constexpr (TEMPORAL && !CARRY) temporal();
    }
    if constexpr (CARRY) {
        __shared__ uint2 ldsStack[kLdsStackDepth * 256];
        const DIVisArgs* va = di_vis_args(extra...);
        #pragma unroll
        for (int trip = 0; trip < (RAYTRACED ? 2 : 1); trip++) {
            bool blocked = false;
            if (want) { float dist; v3 vis; blocked = di_shadow_ray(va->bv, va->ac, va->counters, ldsStack, s.P, target, dist, vis); }
            want = false;
            if (trip == 1) { if (blocked) pPrev = 0.0f; continue; }
            if (blocked) res = di_empty(di_candidates<BRDF>(a));                               // initial visibility
            if (TEMPORAL && valid) temporal();
        }
    }
    if (basicPending) {
        const float p = res.TargetPdf;
        const float den = p * ((float)Mcur * p + (float)MH * pPrev);
        res.W = den > 0.0f ? wsum * (fromH ? pPrev : p) / den : 0.0f;
    }
    if (TEMPORAL && r.boiling) di_boiling(r, valid, res);
    if (inside) di_store<CARRY>(r.out, pi, res);
}

// Spatial reuse, then final shading in the same thread. SPATIAL = false: the final reservoir is the input (temporal-only).
// VIS & kDIVisRaytraced (with BASIC): in the normalisation a neighbour's p counts as 0 when the ray from that neighbour's surface to the
// selected sample is blocked -- one trace site inside that loop.
// BIAS = kDIBiasPairwise: the neighbours stream through one loop with their pairwise weights, the centre (the canonical domain) is merged
// last with the share the slots left it, and there is no second loop.
template <bool SPATIAL, uint32_t BIAS, uint32_t VIS, typename... Extra>
__global__ __launch_bounds__(256) void k_di_spatial_shade(DIReuseArgs r, BlobView bv, AlphaContext ac, DeviceCounters* counters, Extra... extra)
{
    constexpr bool BASIC = BIAS == kDIBiasBasic, PAIRWISE = BIAS == kDIBiasPairwise;
    constexpr bool CARRY = VIS != 0u;
    static_assert(!PAIRWISE || (SPATIAL && !(VIS & kDIVisRaytraced)), "pairwise traces nothing and belongs to a pass that is on");
    __shared__ uint2 ldsStack[kLdsStackDepth * 256];
    const DIArgs& a = r.d;
    uint32_t x, y; di_pixel(x, y);
    if (x >= a.fv.width || y >= a.fv.localRows) return;                 // no barrier below
    const size_t pi = (size_t)y * a.fv.width + x;
    PtDIReservoir c = di_load<CARRY>(r.in, pi);
    DISurface s;
    if (!di_surface(a, a.view, pi, x, y, s)) { di_store<CARRY>(r.out, pi, c); return; }
    if constexpr (PAIRWISE) {
        const int w = (int)a.fv.width;
        uint32_t rng = ml_hash(rng_init(x, y, a.frameIndex) ^ kDISpatialSalt);
        const uint32_t start = (uint32_t)(rng_float(rng) * 8191.0f);
        const uint32_t n = c.M < r.maxHistory ? max(r.spatialSamples, r.boostSamples) : r.spatialSamples;
        const float nf = (float)n, inv = 1.0f / (nf + 1.0f);
        float wsum = 0.0f, own = 0.0f, pSel = 0.0f;
        uint32_t M = c.M, k = 0u;
        int sel = -1;                                                     // the selected neighbour's pixel: its reservoir is loaded again after
                                                                          // the loop. Kept in registers through the loop the selected sample
                                                                          // costs the kernel a wave per SIMD (138 VGPRs against 127)
        for (uint32_t i = 0; i < n; i++) {
            int qx, qy;
            if (!di_neighbour(r, x, y, start, i, qx, qy)) continue;
            DISurface sn;
            if (!di_surface(a, a.view, (size_t)qy * w + qx, qx, qy, sn)) continue;
            if (!di_similar(s, sn, s.depth, r.sNormal, r.sDepth)) continue;
            k++;
            const float pic = di_target_of(a, sn, c.LightIndex, c.U, c.V);       // the centre's sample at the neighbour: sn's last use
            const PtDIReservoir rn = di_load<CARRY>(r.in, (size_t)qy * w + qx);
            const float pn = di_target_of(a, s, rn.LightIndex, rn.U, rn.V);
            const float rc = rng_float(rng);
            const float nM = nf * (float)rn.M;
            const float wn = di_pair_share(nM * rn.TargetPdf, (float)c.M * pn) * inv * pn * rn.W;
            own += di_pair_share((float)c.M * c.TargetPdf, nM * pic);
            wsum += wn; M += rn.M;
            if (rc * wsum < wn) { sel = qy * w + qx; pSel = pn; }
        }
        if (k) {                                                         // no contributing slot: the centre as it is
            const float wc = (1.0f + (float)(n - k) + own) * inv * c.TargetPdf * c.W;
            wsum += wc;
            if (rng_float(rng) * wsum < wc) { sel = -1; pSel = c.TargetPdf; }
            if (sel >= 0) {
                const PtDIReservoir rn = di_load<CARRY>(r.in, (size_t)sel);
                c.LightIndex = rn.LightIndex; c.U = rn.U; c.V = rn.V; c.Age = rn.Age;
                if (CARRY) c.Visibility = di_vis_carry(rn.Visibility, sel % w - (int)x, sel / w - (int)y, 0u);
            }
            if (pSel > 0.0f) { c.M = M; c.TargetPdf = pSel; c.W = wsum / pSel; } else c = di_empty(M);
        }
    } else if (SPATIAL) {
        const int w = (int)a.fv.width;
        uint32_t rng = ml_hash(rng_init(x, y, a.frameIndex) ^ kDISpatialSalt);
        const uint32_t start = (uint32_t)(rng_float(rng) * 8191.0f);
        const uint32_t n = c.M < r.maxHistory ? max(r.spatialSamples, r.boostSamples) : r.spatialSamples;
        float wsum = c.TargetPdf * c.W * (float)c.M;                       // combine(s, centre, 0.5, p(y_c)): selects the centre
        uint32_t M = c.M, mask = 0u;
        int sel = -1;
        PtDIReservoir o = c;
        for (uint32_t i = 0; i < n; i++) {
            int qx, qy;
            if (!di_neighbour(r, x, y, start, i, qx, qy)) continue;
            DISurface sn;
            if (!di_surface(a, a.view, (size_t)qy * w + qx, qx, qy, sn)) continue;
            if (!di_similar(s, sn, s.depth, r.sNormal, r.sDepth)) continue;
            mask |= 1u << i;
            const PtDIReservoir rn = di_load<CARRY>(r.in, (size_t)qy * w + qx);
            const float pn = di_target_of(a, s, rn.LightIndex, rn.U, rn.V);
            const float rc = rng_float(rng);
            const float wn = pn * rn.W * (float)rn.M;
            wsum += wn; M += rn.M;
            if (rc * wsum < wn) { o.LightIndex = rn.LightIndex; o.U = rn.U; o.V = rn.V; o.TargetPdf = pn; o.Age = rn.Age; sel = (int)i;
                if (CARRY) o.Visibility = di_vis_carry(rn.Visibility, qx - (int)x, qy - (int)y, 0u);
            }
        }
        const float p = o.TargetPdf;
        o.M = M;
        if (p > 0.0f) {
            if (BASIC) {                                                     // sum over the centre and the contributing neighbours
                float den = (float)c.M * p, pSrc = p;
                v3 posSel = V3(0.0f, 0.0f, 0.0f);
                if constexpr ((VIS & kDIVisRaytraced) != 0u) posSel = di_sample_point(a, o.LightIndex, o.U, o.V);
                for (uint32_t i = 0; i < n; i++) {
                    if (!(mask & (1u << i))) continue;
                    int qx, qy;
                    di_neighbour(r, x, y, start, i, qx, qy);                 // inside: the first loop took it
                    DISurface sn;
                    di_surface(a, a.view, (size_t)qy * w + qx, qx, qy, sn);
                    float pn = di_target_of(a, sn, o.LightIndex, o.U, o.V);
                    if constexpr ((VIS & kDIVisRaytraced) != 0u) {
                        float dist; v3 vis;
                        if (pn > 0.0f && di_shadow_ray(bv, ac, counters, ldsStack, sn.P, posSel, dist, vis)) pn = 0.0f;
                    }
                    den += (float)r.in[(size_t)qy * w + qx].M * pn;
                    if ((int)i == sel) pSrc = pn;
                }
                den *= p;
                o.W = den > 0.0f ? wsum * pSrc / den : 0.0f;
            } else {
                o.W = wsum / (p * (float)M);
            }
        } else {
            o = di_empty(M);
        }
        c = o;
    }
    // final shading. The stored reservoir is the final one: next frame's history. With the visibility word a young, nearby one stands in
    // for the ray and the reservoir is stored as it is; otherwise the traced visibility is stored (d = 0, age 0). Without the word the
    // ray changes nothing in the reservoir, which is stored ahead of it.
    const bool lit = c.LightIndex < a.count && c.W > 0.0f;
    if (!CARRY || !lit) di_store<CARRY>(r.out, pi, c);
    if (!lit) return;
    v3 pos, dif, spc, vis;
    float power, dist;
    const float W = c.W;
    di_target(a, s, c.LightIndex, c.U, c.V, pos, dif, spc, power);
    bool reuse = false;
    if constexpr (CARRY) { const DIVisArgs* va = di_vis_args(extra...); reuse = va->maxAge != 0u && di_vis_reusable(c.Visibility, va->maxAge, va->maxDistance); }
    if (reuse) {
        const v3 d = pos - s.P;
        dist = sqrtf(dot(d, d));
        vis = di_vis_colour(c.Visibility);
    } else {
        di_shadow_ray(bv, ac, counters, ldsStack, s.P, pos, dist, vis);
        if constexpr (CARRY) {
            c.Visibility = di_vis_pack(vis);
            if (di_vis_args(extra...)->discard != 0u && vis.x == 0.0f && vis.y == 0.0f && vis.z == 0.0f) c = di_empty(c.M);
        }
    }
    if constexpr (CARRY) di_store<true>(r.out, pi, c);
    di_final_write(a, pi, dist, vis, dif, spc, W);
}

// ---- host --------------------------------------------------------------------------------------------------------------------
// The spatial neighbour-offset table: the R2 sequence from (0.5, 0.5), points outside the disc of radius 0.5
// rejected, scaled to int8. Built in double on the host, the same on every machine.
void build_di_offsets(int8_t* out)
{
    const double phi = 1.0 / 1.3247179572447, phi2 = phi * phi;
    double u = 0.5, v = 0.5;
    for (uint32_t k = 0; k < kDIOffsetCount;) {
        u += phi; v += phi2;
        if (u >= 1.0) u -= 1.0;
        if (v >= 1.0) v -= 1.0;
        if ((u - 0.5) * (u - 0.5) + (v - 0.5) * (v - 0.5) > 0.25) continue;
        out[2 * k] = (int8_t)(int)((u - 0.5) * 254.0);
        out[2 * k + 1] = (int8_t)(int)((v - 0.5) * 254.0);
        k++;
    }
}

// The scene's light list, one per context (a context that views another's scene lists the same triangles from the owner's read-only
// top-level inputs, on its own stream; no context writes another's list). Rebuilt when the instances of the top level, the object-data
// binding or pt_invalidate_object_data change it: two small kernels and one wait for the count. Nothing else waits.
hipError_t ensure_light_list(Context& c, const SceneView& sv)
{
    const Context& s = c.sceneOwner ? *c.sceneOwner : c;            // who built the top level: the hash of its instances
    uint64_t key = 1469598103934665603ull;
    auto mix = [&](uint64_t v) { key = (key ^ v) * 1099511628211ull; };
    mix(s.tlasLightHash); mix(c.scene.instanceCount); mix((uint64_t)(uintptr_t)c.scene.instSource); mix((uint64_t)(uintptr_t)c.objects); mix(c.objectCount);
    mix(c.objectDataGen);
    if (c.lightListValid && c.lightListKey == key) return hipSuccess;
    hipError_t e;
    const uint32_t n = c.scene.instanceCount;
    c.lightCount = 0; c.lightListValid = false; c.diHistoryValid = false;       // light indices may move
    if (n && c.scene.instSource && c.scene.blasTable && c.objectCount) {
        if ((e = grow(c.stream, nullptr, want(c.lightInstStart, n + 1u))) != hipSuccess) return e;
        k_light_count<<<1, 1024, 0, c.stream>>>(c.scene.instSource, c.scene.blasTable, n, sv.objects, sv.heap, c.lightInstStart.data());
        uint32_t total = 0;
        if ((e = hipMemcpyAsync(&total, c.lightInstStart.data() + n, sizeof total, hipMemcpyDeviceToHost, c.stream)) != hipSuccess) return e;
        if ((e = hipStreamSynchronize(c.stream)) != hipSuccess) return e;
        if ((e = grow(c.stream, nullptr, want(c.lightList, total), want(c.lightFirst, c.objectCount))) != hipSuccess) return e;
        if ((e = hipMemsetAsync(c.lightFirst.data(), 0xFF, sizeof(uint32_t) * c.objectCount, c.stream)) != hipSuccess) return e;
        if (total) k_light_fill<<<n, 256, 0, c.stream>>>(c.scene.instSource, c.scene.blasTable, sv.objects, sv.heap, c.lightInstStart.data(), c.lightList.data(),
                                                         c.lightFirst.data(), c.objectCount);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        c.lightCount = total;
    }
    c.lightListKey = key; c.lightListValid = true;
    return hipSuccess;
}

} // namespace pt

using namespace pt;

// ---- pt_di_render_with_history, in stages ----------------------------------------------------------------------------------
// the arguments, checked in this order
static int di_check_args(Context& c, const PtTextures* tx, const PtDIPreviousTextures* prev)
{
    API_ARG(&c, tx, "textures is NULL");
    if (!c.haveDISettings) return fail(&c, PT_ERROR_NOT_READY, "call pt_di_set_constants first");
    const PtDISettings& s = c.diSettings;
    const bool empty = !rank_holds_pixels(c, s.RenderSize[0], s.RenderSize[1]);            // a rank without rows: nothing to bind, nothing is launched
    API_ARG(&c, empty || (tx->LinearDepth && tx->GeometricNormal && tx->NormalRoughness && tx->BaseColorMetalness && tx->IOR && tx->Transmission),
           "a G-buffer texture the DI pass reads is not bound (LinearDepth, GeometricNormal, NormalRoughness, BaseColorMetalness, IOR, Transmission)");
    const bool toRadiance = s.IsLastRenderPass && s.Denoiser <= PT_DENOISER_DLSS_RAY_RECONSTRUCTION;
    API_ARG(&c, empty || (toRadiance ? tx->Radiance != nullptr : (tx->Diffuse && tx->Specular)),
           toRadiance ? "IsLastRenderPass with Denoiser None / DLSS-RR adds to Textures.Radiance: not bound" : "the DI pass writes Textures.Diffuse / Textures.Specular: not bound");
    if (!empty && c.diReuseOn && c.diReuse.TemporalResampling)
        API_ARG(&c, prev && prev->PreviousGeometricNormal && prev->PreviousLinearDepth && prev->PreviousBaseColorMetalness && prev->PreviousNormalRoughness &&
               prev->PreviousIOR && prev->PreviousTransmission && tx->MotionVector,
               "temporal resampling reads Textures.MotionVector and the six Previous* textures: not bound");
    if (c.diReuseOn && c.diVisibilityOn) {
        API_ARG(&c, !(c.diVisibility.TemporalRaytraced && c.diReuse.TemporalResampling) || c.diReuse.TemporalBiasCorrection == PT_DI_BIAS_CORRECTION_BASIC,
               "TemporalRaytraced needs TemporalBiasCorrection = PT_DI_BIAS_CORRECTION_BASIC");
        API_ARG(&c, !(c.diVisibility.SpatialRaytraced && c.diReuse.SpatialSamples) || c.diReuse.SpatialBiasCorrection == PT_DI_BIAS_CORRECTION_BASIC,
               "SpatialRaytraced needs SpatialBiasCorrection = PT_DI_BIAS_CORRECTION_BASIC");
    }
    if (c.diReuseOn) {                                                         // a flag on a pass that is off is ignored
        const bool tp = c.diPairwise.TemporalPairwise && c.diReuse.TemporalResampling, sp = c.diPairwise.SpatialPairwise && c.diReuse.SpatialSamples;
        API_ARG(&c, !tp || c.diReuse.TemporalBiasCorrection == PT_DI_BIAS_CORRECTION_BASIC, "TemporalPairwise needs TemporalBiasCorrection = PT_DI_BIAS_CORRECTION_BASIC");
        API_ARG(&c, !sp || c.diReuse.SpatialBiasCorrection == PT_DI_BIAS_CORRECTION_BASIC, "SpatialPairwise needs SpatialBiasCorrection = PT_DI_BIAS_CORRECTION_BASIC");
        API_ARG(&c, !(tp && c.diVisibilityOn && c.diVisibility.TemporalRaytraced), "TemporalPairwise and TemporalRaytraced are two corrections of one pass: set one");
        API_ARG(&c, !(sp && c.diVisibilityOn && c.diVisibility.SpatialRaytraced), "SpatialPairwise and SpatialRaytraced are two corrections of one pass: set one");
    }
    return PT_OK;
}

// (width, height, mips) of the PDF texture of n lights: ComputePdfTextureSize (Source/RTXDIResources.ixx:43-52) in integers
static void di_pdf_size(uint32_t n, uint32_t size[3])
{
    n = std::max(n, 1u);
    uint32_t w = 1, h = 1, mips = 1;
    while ((uint64_t)w * w < n) w <<= 1;                                   // the smallest power of two >= ceil(sqrt(n))
    while ((uint64_t)h * w < n) h <<= 1;                                   // ... >= ceil(n / width)
    for (uint32_t e = std::max(w, h); e > 1u; e >>= 1) mips++;
    size[0] = w; size[1] = h; size[2] = mips;
}
static uint32_t di_pdf_level_texels(const uint32_t size[3], uint32_t k) { return std::max(1u, size[0] >> k) * std::max(1u, size[1] >> k); }
static uint32_t di_pdf_texels(const uint32_t size[3])
{
    uint32_t t = 0;
    for (uint32_t k = 0; k < size[2]; k++) t += di_pdf_level_texels(size, k);
    return t;
}
// whether the descent of the PDF texture replaces the prefix sum in this render's candidates (and a.total becomes top * M * M)
static bool di_pdf_acts(const Context& c)
{
    return c.diPdfMipmap && (c.diSampling.Mode == PT_DI_LOCAL_LIGHT_POWER_RIS || c.diSampling.Mode == PT_DI_LOCAL_LIGHT_REGIR_RIS);
}

// the n light records and the prefix sum of their powers (nb scan blocks); the total lands in lightBlockSums[nb]. With pt_di_set_pdf_mipmap on,
// the PDF texture and its chain too; where it acts nothing of the render reads the prefix sum, and its three launches are skipped.
static int di_light_records(Context& c, const SceneView& sv, uint32_t n, uint32_t nb)
{
    API_HIP(&c, grow(c.stream, nullptr, want(c.lightRecords, n), want(c.lightCdf, (size_t)n * 2u), want(c.lightBlockSums, nb + 1u)));
    float* power = c.lightCdf.data() + c.lightCdf.capacity() / 2u;        // cdf | powers: the halves of the one buffer, whatever else grew with it
    k_light_records<<<(n + 255u) / 256u, 256, 0, c.stream>>>(c.lightList.data(), n, c.scene.instSource, sv.objects, sv.heap, sv.shadeTex, sv.srgbLut, (float4*)c.lightRecords.data(), power);
    if (!di_pdf_acts(c)) {
        k_cdf_local<<<nb, 256, 0, c.stream>>>(power, n, c.lightCdf.data(), c.lightBlockSums.data());
        k_cdf_blocks<<<1, 1, 0, c.stream>>>(c.lightBlockSums.data(), nb);
        k_cdf_add<<<(n + 255u) / 256u, 256, 0, c.stream>>>(c.lightCdf.data(), n, c.lightBlockSums.data(), nb);
    }
    if (!c.diPdfMipmap) return PT_OK;
    API_ARG(&c, n <= (1u << 24), "the PDF texture holds at most 2^24 lights");
    uint32_t size[3];
    di_pdf_size(n, size);
    const uint32_t texels = di_pdf_texels(size);
    API_HIP(&c, grow(c.stream, nullptr, want(c.diPdfTexture, (size_t)texels + 1u)));
    float* levels[16];
    uint32_t at = 0;
    for (uint32_t k = 0; k < size[2]; k++) { levels[k] = c.diPdfTexture.data() + at; at += di_pdf_level_texels(size, k); }
    k_pdf_level0<<<(size[0] * size[1] + 255u) / 256u, 256, 0, c.stream>>>(power, n, size[0], size[0] * size[1], levels[0]);
    API_HIP(&c, hipGetLastError());
    const int st = mip_generate(c, levels, size[0], size[1], size[2]);
    if (st != PT_OK) return st;
    k_pdf_denominator<<<1, 1, 0, c.stream>>>(levels[size[2] - 1u], (float)std::max(size[0], size[1]), c.diPdfTexture.data() + texels);
    API_HIP(&c, hipGetLastError());
    memcpy(c.diPdfSize, size, sizeof size);
    return PT_OK;
}

// The Onion layout's tables, built once in double and stored as float.
static const OnionTables& onion_tables()
{
    static const OnionTables tables = [] {
        static const uint32_t groupLayers[kOnionGroups] = { 1, 1, 1, 1, 11 };
        const double pi = 3.14159265358979323846;
        OnionTables t; memset(&t, 0, sizeof t);
        uint32_t nRing = 0, nAz = 0, cell = 1, layer = 0;
        double B = 1.0;
        t.cells[0] = make_float4(0.0f, 0.0f, 0.0f, 1.0f);
        t.b2[0] = 1.0f;
        auto point = [](double r, double E, double A, double* o) { o[0] = r * cos(E) * cos(A); o[1] = r * sin(E); o[2] = r * cos(E) * sin(A); };
        auto dist = [](const double* a, const double* b) { return sqrt((a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1]) + (a[2] - b[2]) * (a[2] - b[2])); };
        for (uint32_t g = 0; g < kOnionGroups; g++) {
            const uint32_t p = 8u + 4u * g, rings = p / 4u + 1u;
            const double eq = 2.0 * pi / p, ratio = (p + pi) / (p - pi);
            for (uint32_t k = 1; k < rings; k++) {
                const double sn = sin((k - 0.5) * eq);
                const uint32_t before = kOnionRingCells[g][k - 1u];
                t.ringStep[nRing] = (k == 1u ? before : 2u * before) | ((before - 1u) << 8) | (kOnionRingCells[g][k] << 16);
                t.ring[nRing++] = (float)(sn * sn);
            }
            assert(onion_group_azimuth(g) == nAz && kOnionRingCells[g][0] == p);
            for (uint32_t k = 0; k < rings; k++) {
                const uint32_t n = kOnionRingCells[g][k];
                for (uint32_t j = 1; j < n; j++) {                           // diamond(cos a, sin a) in double
                    const double x = cos(2.0 * pi * j / n), z = sin(2.0 * pi * j / n);
                    t.azimuth[nAz++] = (float)(z >= 0.0 ? (x >= 0.0 ? z / (x + z) : 1.0 + (-x) / (z - x)) : (x < 0.0 ? 2.0 + (-z) / (-x - z) : 3.0 + x / (x - z)));
                }
            }
            for (uint32_t l = 0; l < groupLayers[g]; l++, layer++) {
                const double rIn = B, rOut = B * ratio, rMid = 0.5 * (rIn + rOut);
                assert(onion_layer_base(layer) == cell);
                for (uint32_t k = 0; k < rings; k++) {
                    const uint32_t n = kOnionRingCells[g][k];
                    const double lo = (k - 0.5) * eq, hi = k + 1u == rings ? 0.5 * pi : (k + 0.5) * eq, mid = k ? k * eq : 0.0;
                    for (uint32_t south = 0; south < (k ? 2u : 1u); south++) {
                        const double sgn = south ? -1.0 : 1.0;
                        for (uint32_t i = 0; i < n; i++, cell++) {
                            double c[3], q[3], radius = 0.0;
                            if (n == 1u) {                                   // a polar cap
                                c[0] = 0.0; c[1] = sgn * rMid; c[2] = 0.0;
                                radius = rOut - rMid;
                                for (double r : { rIn, rOut }) { point(r, sgn * lo, 0.0, q); radius = std::max(radius, dist(c, q)); }
                            } else {
                                const double aLo = i * 2.0 * pi / n, aHi = (i + 1u) * 2.0 * pi / n;
                                point(rMid, sgn * mid, (i + 0.5) * 2.0 * pi / n, c);
                                for (double r : { rIn, rOut }) for (double E : { lo, hi }) for (double A : { aLo, aHi }) { point(r, sgn * E, A, q); radius = std::max(radius, dist(c, q)); }
                            }
                            t.cells[cell] = make_float4((float)c[0], (float)c[1], (float)c[2], (float)radius);
                        }
                    }
                }
                B = rOut;
                t.b2[layer + 1u] = (float)(B * B);
            }
        }
        assert(nRing == kOnionRings && nAz == kOnionAzimuths && cell == kOnionCells && layer == kOnionLayers);
        return t;
    }();
    return tables;
}

// local-light sampling: Power_RIS tiles (POWER_RIS, REGIR_RIS), then the ReGIR cells around this render's camera (REGIR_RIS) in the
// context's layout; ls is the candidate source of every mode but POWER_CDF
static int di_presample(Context& c, uint32_t n, uint32_t nb, DISampling& ls)
{
    const PtDILightSamplingSettings& lss = c.diSampling;
    memset(&ls, 0, sizeof ls);
    ls.mode = lss.Mode;
    if (lss.Mode != PT_DI_LOCAL_LIGHT_POWER_RIS && lss.Mode != PT_DI_LOCAL_LIGHT_REGIR_RIS) return PT_OK;
    const bool regir = lss.Mode == PT_DI_LOCAL_LIGHT_REGIR_RIS, onion = regir && c.diReGIRLayout == PT_DI_REGIR_LAYOUT_ONION;
    const uint32_t cellEntries = onion ? kDIOnionEntries : kDICellEntries;                    // 9.2 MB or 16 MB, only in ReGIR mode
    API_HIP(&c, grow(c.stream, nullptr, want(c.diTiles, kDITileEntries), want(c.diCells, regir ? cellEntries : 0u)));
    if (onion) API_HIP(&c, upload_once(c.diOnion, &onion_tables(), sizeof(OnionTables)));
    if (di_pdf_acts(c))
        k_di_presample_tiles_mip<<<kDITileEntries / 256u, 256, 0, c.stream>>>(c.diPdfTexture.data(), c.diPdfSize[0], c.diPdfSize[1], c.diPdfSize[2], di_pdf_texels(c.diPdfSize),
                                                                             n, c.diSettings.FrameIndex, (uint2*)c.diTiles.data());
    else
        k_di_presample_tiles<<<kDITileEntries / 256u, 256, 0, c.stream>>>((const float4*)c.lightRecords.data(), c.lightCdf.data(), c.lightBlockSums.data() + nb, n,
                                                                         c.diSettings.FrameIndex, (uint2*)c.diTiles.data());
    API_HIP(&c, hipGetLastError());
    c.diTileCount = kDITileEntries;
    ls.tiles = (const uint2*)c.diTiles.data();
    if (regir) {
        memcpy(ls.centre, c.camera.Position, sizeof ls.centre);
        ls.cellSize = lss.ReGIRCellSize;
        if (onion) {
            ls.layout = PT_DI_REGIR_LAYOUT_ONION;
            ls.onion = (const OnionTables*)c.diOnion.data();
            k_di_regir_build_onion<<<kDIOnionEntries / 256u, 256, 0, c.stream>>>((const float4*)c.lightRecords.data(), n, ls.tiles, ls.onion, ls.centre[0], ls.centre[1],
                                                                                ls.centre[2], 0.5f * ls.cellSize, lss.ReGIRBuildSamples, c.diSettings.FrameIndex,
                                                                                (uint2*)c.diCells.data());
        } else
            k_di_regir_build<<<kDICellEntries / 256u, 256, 0, c.stream>>>((const float4*)c.lightRecords.data(), n, ls.tiles, ls.centre[0], ls.centre[1], ls.centre[2],
                                                                          ls.cellSize, lss.ReGIRBuildSamples, c.diSettings.FrameIndex, (uint2*)c.diCells.data());
        API_HIP(&c, hipGetLastError());
        c.diCellCount = cellEntries;
        ls.cells = (const uint2*)c.diCells.data();
    }
    return PT_OK;
}

static DIView di_view(const DIGBuffer& g, const float* projectionToView, const float* viewToWorld, const float* position)
{
    DIView v; v.g = g;
    memcpy(v.projectionToView, projectionToView, sizeof v.projectionToView); memcpy(v.viewToWorld, viewToWorld, sizeof v.viewToWorld);
    memcpy(v.position, position, sizeof v.position);
    return v;
}

// calls f with the candidate source of the light-sampling mode: the kernels that draw candidates are instantiated for each source
template <typename F> static void di_with_source(const DISampling& ls, F&& f)
{
    if (ls.mode == PT_DI_LOCAL_LIGHT_POWER_CDF) f(DIPowerCDF{});
    else f(ls);
}

// calls f with the compile-time form of a reuse pass, (pass on, BIAS, VIS), and with va behind it when VIS != 0. The forms are
// {(0, Off), (1, Off), (1, Basic), (1, Pairwise)} x {0, kDIVisOn} and (1, Basic, kDIVisOn | kDIVisRaytraced): di_check_args refuses raytraced
// and pairwise without Basic, and the two together.
template <typename F> static void di_with_form(bool on, bool basic, bool pairwise, bool vis, bool raytraced, const DIVisArgs& va, F&& f)
{
    using std::integral_constant;
    auto with_vis = [&](auto ON, auto BIAS) {
        if (vis) f(ON, BIAS, integral_constant<uint32_t, kDIVisOn>{}, va);
        else f(ON, BIAS, integral_constant<uint32_t, 0u>{});
    };
    using Off = integral_constant<uint32_t, kDIBiasOff>; using Basic = integral_constant<uint32_t, kDIBiasBasic>;
    if (!on) with_vis(std::false_type{}, Off{});
    else if (raytraced) f(std::true_type{}, Basic{}, integral_constant<uint32_t, kDIVisOn | kDIVisRaytraced>{}, va);
    else if (pairwise) with_vis(std::true_type{}, integral_constant<uint32_t, kDIBiasPairwise>{});
    else if (basic) with_vis(std::true_type{}, Basic{});
    else with_vis(std::true_type{}, Off{});
}

// reservoir reuse: k_di_initial_temporal (last frame's B -> A), k_di_spatial_shade (A -> B); B is next frame's history
static int di_launch_reuse(Context& c, const DIArgs& a, const DISampling& ls, const PtDIPreviousTextures* prev, dim3 grid, const AlphaContext& ac)
{
    const PtDIResamplingSettings& rs = c.diReuse;
    const bool temporal = rs.TemporalResampling, spatial = rs.SpatialSamples > 0;
    const FrameView& fv = a.fv;
    const size_t npix = (size_t)fv.width * fv.localRows;
    bool grew = false;
    API_HIP(&c, grow(c.stream, &grew, want(c.diResA, npix), want(c.diResB, npix)));
    if (grew) c.diHistoryValid = false;
    if (!c.diOffsets) {
        int8_t host[2 * kDIOffsetCount];
        build_di_offsets(host);
        API_HIP(&c, upload_once(c.diOffsets, host, sizeof host));
    }
    if (c.diHistorySize[0] != fv.width || c.diHistorySize[1] != fv.height || c.diHistoryLightKey != c.lightListKey) c.diHistoryValid = false;
    DIReuseArgs r; memset(&r, 0, sizeof r);
    r.d = a;
    if (temporal)
        r.prev = di_view(DIGBuffer{ prev->PreviousLinearDepth, prev->PreviousNormalRoughness, prev->PreviousGeometricNormal, prev->PreviousBaseColorMetalness,
                                    prev->PreviousIOR, prev->PreviousTransmission },
                         c.camera.PreviousProjectionToView, c.camera.PreviousViewToWorld, c.camera.PreviousPosition);
    r.offsets = (const char2*)c.diOffsets.data();
    r.haveHistory = c.diHistoryValid ? 1u : 0u;
    r.maxHistory = rs.MaxHistoryLength; r.boiling = rs.BoilingFilter; r.spatialSamples = rs.SpatialSamples; r.boostSamples = rs.DisocclusionBoostSamples;
    r.boilingMul = 10.0f / std::min(std::max(rs.BoilingFilterStrength, 1e-6f), 1.0f) - 9.0f;
    r.tDepth = rs.TemporalDepthThreshold; r.tNormal = rs.TemporalNormalThreshold;
    r.radius = rs.SpatialSamplingRadius; r.sDepth = rs.SpatialDepthThreshold; r.sNormal = rs.SpatialNormalThreshold;
    r.in = c.diResB.data(); r.out = c.diResA.data();
    const bool tb = rs.TemporalBiasCorrection == PT_DI_BIAS_CORRECTION_BASIC, sb = rs.SpatialBiasCorrection == PT_DI_BIAS_CORRECTION_BASIC;
    const PtDIVisibilitySettings& vs = c.diVisibility;
    const bool vis = c.diVisibilityOn, tr = vis && temporal && vs.TemporalRaytraced, sr = vis && spatial && vs.SpatialRaytraced;
    const bool tp = temporal && c.diPairwise.TemporalPairwise, sp = spatial && c.diPairwise.SpatialPairwise;
    DIVisArgs va; memset(&va, 0, sizeof va);
    va.bv = c.scene.blob; va.ac = ac; va.counters = c.counters.data();
    va.initial = vs.InitialVisibility; va.maxAge = vs.FinalVisibilityReuse ? vs.FinalVisibilityMaxAge : 0u; va.discard = vs.DiscardInvisibleSamples;
    va.maxDistance = vs.FinalVisibilityMaxDistance;
    di_with_source(ls, [&](auto source) {
        di_with_form(temporal, tb, tp, vis, tr, va, [&](auto T, auto B, auto V, auto... extra) {
            if (a.brdfSamples) k_di_initial_temporal<T(), B(), V(), true, decltype(source)><<<grid, 256, 0, c.stream>>>(r, source, extra...);
            else k_di_initial_temporal<T(), B(), V(), false, decltype(source)><<<grid, 256, 0, c.stream>>>(r, source, extra...);
        });
    });
    API_HIP(&c, hipGetLastError());
    r.in = c.diResA.data(); r.out = c.diResB.data();
    di_with_form(spatial, sb, sp, vis, sr, va, [&](auto S, auto B, auto V, auto... extra) {
        k_di_spatial_shade<S(), B(), V()><<<grid, 256, 0, c.stream>>>(r, c.scene.blob, ac, c.counters.data(), extra...);
    });
    API_HIP(&c, hipGetLastError());
    c.diHistoryValid = true; c.diHistorySize[0] = fv.width; c.diHistorySize[1] = fv.height; c.diHistoryLightKey = c.lightListKey;
    c.diResCount = (uint32_t)npix;
    return PT_OK;
}

extern "C" {

int pt_di_set_constants(PtContext* ctx, const PtDISettings* s)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    Context& c = ctx->c;
    API_ARG(&c, s, "settings is NULL");
    API_ARG(&c, s->LocalLightSamples >= 1 && s->LocalLightSamples <= 32, "LocalLightSamples must be 1..32");
    API_ARG(&c, s->Denoiser <= PT_DENOISER_NRD_RELAX, "unknown Denoiser value");
    c.diSettings = *s; c.haveDISettings = true;
    return PT_OK;
}

int pt_di_render_with_history(PtContext* ctx, const PtTextures* tx, const PtDIPreviousTextures* prev)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    Context& c = ctx->c;
    int st = di_check_args(c, tx, prev);
    if (st != PT_OK) return st;
    const PtDISettings& s = c.diSettings;
    const bool reuse = c.diReuseOn;
    API_HIP(&c, hipSetDevice(c.device));
    SceneView sv; FrameView fv; memset(&sv, 0, sizeof sv); memset(&fv, 0, sizeof fv);
    if ((st = make_views(c, s.RenderSize[0], s.RenderSize[1], sv, fv, true)) != PT_OK) return st;
    API_ARG(&c, !reuse || fv.rankCount == 1, "reservoir reuse needs an unsharded context (RankCount 1)");
    const size_t npix = (size_t)fv.width * fv.localRows;
    if (tx->Diffuse) API_HIP(&c, hipMemsetAsync(tx->Diffuse, 0, npix * 8u, c.stream));                // App.cpp:1238-1239
    if (tx->Specular) API_HIP(&c, hipMemsetAsync(tx->Specular, 0, npix * 8u, c.stream));
    API_HIP(&c, ensure_light_list(c, sv));
    const uint32_t n = c.lightCount;
    c.lightRecordCount = n;
    c.diTileCount = 0; c.diCellCount = 0; c.diBrdfCount = 0; memset(c.diPdfSize, 0, sizeof c.diPdfSize);
    if (!reuse || n == 0 || npix == 0) { c.diHistoryValid = false; c.diResCount = 0; }
    if (n == 0 || npix == 0) return PT_OK;
    const uint32_t nb = (n + kScanBlock - 1u) / kScanBlock;
    if ((st = di_light_records(c, sv, n, nb)) != PT_OK) return st;
    DISampling ls;
    if ((st = di_presample(c, n, nb, ls)) != PT_OK) return st;
    DIArgs a; memset(&a, 0, sizeof a);
    a.fv = fv; a.tx = *tx;
    a.view = di_view(DIGBuffer{ tx->LinearDepth, tx->NormalRoughness, tx->GeometricNormal, tx->BaseColorMetalness, tx->IOR, tx->Transmission },
                     c.camera.ProjectionToView, c.camera.ViewToWorld, c.camera.Position);
    memcpy(a.jitter, c.camera.Jitter, sizeof a.jitter);
    a.lights = (const float4*)c.lightRecords.data(); a.cdf = c.lightCdf.data(); a.total = c.lightBlockSums.data() + nb; a.count = n;
    if (di_pdf_acts(c)) a.total = c.diPdfTexture.data() + di_pdf_texels(c.diPdfSize);       // top * M * M: the gate of the pass and the denominator of light_pdf
    a.frameIndex = s.FrameIndex; a.samples = s.LocalLightSamples; a.denoiser = s.Denoiser; a.lastPass = s.IsLastRenderPass; a.ext = s.ExtFlags;
    const AlphaContext ac = alpha_context(sv);
    const dim3 grid((fv.width + 15u) / 16u, (fv.localRows + 15u) / 16u);
    if (c.diBrdf.BrdfSamples) {                                               // the BRDF candidates' rays, ahead of whichever pass draws the candidates
        const size_t nrec = npix * c.diBrdf.BrdfSamples;
        API_HIP(&c, grow(c.stream, nullptr, want(c.diBrdfRecords, nrec)));
        a.brdfSamples = c.diBrdf.BrdfSamples; a.brdfCutoff = c.diBrdf.BrdfCutoff;
        a.brdfRecords = c.diBrdfRecords.data(); a.firstLight = c.lightFirst.data(); a.objectCount = c.objectCount;
        k_di_brdf_rays<<<grid, 256, 0, c.stream>>>(a, c.diBrdfRecords.data(), c.scene.blob, ac, c.counters.data());
        API_HIP(&c, hipGetLastError());
        c.diBrdfCount = (uint32_t)nrec;
    }
    if (reuse) return di_launch_reuse(c, a, ls, prev, grid, ac);
    di_with_source(ls, [&](auto source) {                                     // the plain pass
        if (a.brdfSamples) k_di<decltype(source), true><<<grid, 256, 0, c.stream>>>(a, source, c.scene.blob, ac, c.counters.data());
        else k_di<decltype(source), false><<<grid, 256, 0, c.stream>>>(a, source, c.scene.blob, ac, c.counters.data());
    });
    API_HIP(&c, hipGetLastError());
    return PT_OK;
}

int pt_di_render(PtContext* ctx, const PtTextures* tx) { return pt_di_render_with_history(ctx, tx, nullptr); }

int pt_di_set_resampling(PtContext* ctx, const PtDIResamplingSettings* s)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    Context& c = ctx->c;
    PtDIResamplingSettings v; memset(&v, 0, sizeof v);
    if (s) {
        API_ARG(&c, s->TemporalResampling <= 1u && s->BoilingFilter <= 1u, "TemporalResampling / BoilingFilter must be 0 or 1");
        API_ARG(&c, s->TemporalBiasCorrection != 2u && s->TemporalBiasCorrection != 3u && s->SpatialBiasCorrection != 2u && s->SpatialBiasCorrection != 3u,
               "Pairwise and Raytraced bias correction are not supported (use PT_DI_BIAS_CORRECTION_OFF or _BASIC)");
        API_ARG(&c, s->TemporalBiasCorrection <= 1u && s->SpatialBiasCorrection <= 1u, "unknown bias-correction mode");
        API_ARG(&c, s->MaxHistoryLength >= 1u && s->MaxHistoryLength <= 64u, "MaxHistoryLength must be 1..64");
        API_ARG(&c, s->BoilingFilterStrength >= 0.0f && s->BoilingFilterStrength <= 1.0f, "BoilingFilterStrength must be in [0, 1]");
        API_ARG(&c, s->SpatialSamples <= 32u, "SpatialSamples must be 0..32");
        API_ARG(&c, s->DisocclusionBoostSamples <= 32u, "DisocclusionBoostSamples must be 0..32");
        API_ARG(&c, s->SpatialSamplingRadius > 0.0f && s->SpatialSamplingRadius <= 64.0f, "SpatialSamplingRadius must be in (0, 64]");
        API_ARG(&c, s->TemporalDepthThreshold >= 0.0f && s->SpatialDepthThreshold >= 0.0f && std::isfinite(s->TemporalDepthThreshold) && std::isfinite(s->SpatialDepthThreshold),
               "depth thresholds must be finite and >= 0");
        API_ARG(&c, s->TemporalNormalThreshold >= -1.0f && s->TemporalNormalThreshold <= 1.0f && s->SpatialNormalThreshold >= -1.0f && s->SpatialNormalThreshold <= 1.0f,
               "normal thresholds must be in [-1, 1]");
        v = *s;
        memset(v._pad, 0, sizeof v._pad);
    }
    const bool on = v.TemporalResampling || v.SpatialSamples;
    if (on != c.diReuseOn || memcmp(&v, &c.diReuse, sizeof v) != 0) c.diHistoryValid = false;
    c.diReuse = v; c.diReuseOn = on;
    return PT_OK;
}

int pt_di_set_visibility(PtContext* ctx, const PtDIVisibilitySettings* s)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    Context& c = ctx->c;
    PtDIVisibilitySettings v; memset(&v, 0, sizeof v);
    if (s) {
        API_ARG(&c, s->InitialVisibility <= 1u, "InitialVisibility must be 0 or 1");
        API_ARG(&c, s->FinalVisibilityReuse <= 1u, "FinalVisibilityReuse must be 0 or 1");
        API_ARG(&c, s->DiscardInvisibleSamples <= 1u, "DiscardInvisibleSamples must be 0 or 1");
        API_ARG(&c, s->TemporalRaytraced <= 1u, "TemporalRaytraced must be 0 or 1");
        API_ARG(&c, s->SpatialRaytraced <= 1u, "SpatialRaytraced must be 0 or 1");
        const bool on = s->InitialVisibility || s->FinalVisibilityReuse || s->DiscardInvisibleSamples || s->TemporalRaytraced || s->SpatialRaytraced;
        if (on) {                                                             // all flags 0: the struct is today's behaviour whatever else it holds
            API_ARG(&c, s->FinalVisibilityMaxAge >= 1u && s->FinalVisibilityMaxAge <= 14u, "FinalVisibilityMaxAge must be 1..14");
            API_ARG(&c, s->FinalVisibilityMaxDistance > 0.0f && s->FinalVisibilityMaxDistance <= 31.0f, "FinalVisibilityMaxDistance must be in (0, 31]");
            v = *s;
            v._pad = 0;
        }
    }
    const bool on = v.InitialVisibility || v.FinalVisibilityReuse || v.DiscardInvisibleSamples || v.TemporalRaytraced || v.SpatialRaytraced;
    if (memcmp(&v, &c.diVisibility, sizeof v) != 0) c.diHistoryValid = false;
    c.diVisibility = v; c.diVisibilityOn = on;
    return PT_OK;
}

int pt_di_set_pairwise(PtContext* ctx, const PtDIPairwiseSettings* s)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    Context& c = ctx->c;
    PtDIPairwiseSettings v; memset(&v, 0, sizeof v);
    if (s) {
        API_ARG(&c, s->TemporalPairwise <= 1u, "TemporalPairwise must be 0 or 1");
        API_ARG(&c, s->SpatialPairwise <= 1u, "SpatialPairwise must be 0 or 1");
        API_ARG(&c, s->Reserved[0] == 0u && s->Reserved[1] == 0u, "Reserved must be 0");
        v = *s;
    }
    if (memcmp(&v, &c.diPairwise, sizeof v) != 0) c.diHistoryValid = false;
    c.diPairwise = v;
    return PT_OK;
}

int pt_di_set_light_sampling(PtContext* ctx, const PtDILightSamplingSettings* s)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    Context& c = ctx->c;
    PtDILightSamplingSettings v; memset(&v, 0, sizeof v);
    if (s) {
        API_ARG(&c, s->Mode <= PT_DI_LOCAL_LIGHT_REGIR_RIS, "unknown local-light sampling Mode");
        API_ARG(&c, std::isfinite(s->ReGIRCellSize) && s->ReGIRCellSize >= 0.1f && s->ReGIRCellSize <= 10.0f, "ReGIRCellSize must be finite and in [0.1, 10]");
        API_ARG(&c, s->ReGIRBuildSamples >= 1u && s->ReGIRBuildSamples <= 32u, "ReGIRBuildSamples must be 1..32");
        v = *s;
        v._pad = 0;
    }
    if (memcmp(&v, &c.diSampling, sizeof v) != 0) c.diHistoryValid = false;
    c.diSampling = v;
    return PT_OK;
}

int pt_di_set_regir_layout(PtContext* ctx, const PtDIReGIRLayoutSettings* s)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    Context& c = ctx->c;
    const uint32_t layout = s ? s->Layout : (uint32_t)PT_DI_REGIR_LAYOUT_GRID;
    API_ARG(&c, layout <= PT_DI_REGIR_LAYOUT_ONION, "unknown ReGIR Layout");
    if (layout != c.diReGIRLayout) c.diHistoryValid = false;
    c.diReGIRLayout = layout;
    return PT_OK;
}

int pt_di_set_brdf_sampling(PtContext* ctx, uint32_t brdf_samples, float brdf_cutoff)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    Context& c = ctx->c;
    API_ARG(&c, brdf_samples <= 8u, "brdf_samples must be 0..8");
    API_ARG(&c, std::isfinite(brdf_cutoff) && brdf_cutoff >= 0.0f && brdf_cutoff < 1.0f, "brdf_cutoff must be finite and in [0, 1)");
    Context::DIBrdfSettings v;
    if (brdf_samples) { v.BrdfSamples = brdf_samples; v.BrdfCutoff = brdf_cutoff + 0.0f; }      // 0 samples: off whatever the cutoff; -0 is 0
    if (v.BrdfSamples != c.diBrdf.BrdfSamples || v.BrdfCutoff != c.diBrdf.BrdfCutoff) c.diHistoryValid = false;
    c.diBrdf = v;
    return PT_OK;
}

int pt_di_pdf_texture_size(uint32_t light_count, uint32_t* width, uint32_t* height, uint32_t* mip_levels)
{
    if (!width || !height || !mip_levels || light_count > (1u << 24)) return PT_ERROR_INVALID_ARGUMENT;
    uint32_t size[3];
    di_pdf_size(light_count, size);
    *width = size[0]; *height = size[1]; *mip_levels = size[2];
    return PT_OK;
}

int pt_di_set_pdf_mipmap(PtContext* ctx, uint32_t enabled)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    Context& c = ctx->c;
    API_ARG(&c, enabled <= 1u, "enabled must be 0 or 1");
    if (enabled != c.diPdfMipmap) c.diHistoryValid = false;
    c.diPdfMipmap = enabled;
    return PT_OK;
}

int pt_di_download_pdf_texture(PtContext* ctx, uint32_t level, float* host_dst, uint32_t capacity, uint32_t* out_width, uint32_t* out_height)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    Context& c = ctx->c;
    API_ARG(&c, out_width && out_height && (host_dst || capacity == 0), "out_width / out_height / host_dst is NULL");
    API_ARG(&c, level < 16u, "level must be below 16");
    API_HIP(&c, hipSetDevice(c.device));
    API_HIP(&c, hipStreamSynchronize(c.stream));
    *out_width = 0; *out_height = 0;
    if (level >= c.diPdfSize[2]) return PT_OK;                               // no texture, or no such level of it
    uint32_t at = 0;
    for (uint32_t k = 0; k < level; k++) at += di_pdf_level_texels(c.diPdfSize, k);
    *out_width = std::max(1u, c.diPdfSize[0] >> level); *out_height = std::max(1u, c.diPdfSize[1] >> level);
    const size_t n = std::min((size_t)capacity, (size_t)*out_width * *out_height);
    if (n) API_HIP(&c, hipMemcpy(host_dst, c.diPdfTexture.data() + at, sizeof(float) * n, hipMemcpyDeviceToHost));
    return PT_OK;
}

int pt_di_download_brdf_candidates(PtContext* ctx, uint32_t* host_dst, uint32_t capacity, uint32_t* out_count)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    Context& c = ctx->c;
    API_ARG(&c, out_count && (host_dst || capacity == 0), "out_count / host_dst is NULL");
    return download_counted(c, c.diBrdfRecords.data(), c.diBrdfCount, 1u, (uint4*)host_dst, capacity, out_count);
}

int pt_di_regir_onion_table(uint32_t which, float* host_dst, uint32_t capacity, uint32_t* out_count)
{
    if (!out_count || (!host_dst && capacity) || which > 3u) return PT_ERROR_INVALID_ARGUMENT;
    const OnionTables& t = onion_tables();
    const float* src[4] = { t.b2, t.ring, t.azimuth, &t.cells[0].x };
    const uint32_t count[4] = { 16u, kOnionRings, kOnionAzimuths, 4u * kOnionCells };
    *out_count = count[which];
    if (capacity) memcpy(host_dst, src[which], sizeof(float) * std::min(capacity, count[which]));
    return PT_OK;
}

int pt_di_download_presampled(PtContext* ctx, uint32_t which, PtDIPresampledLight* host_dst, uint32_t capacity, uint32_t* out_count)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    Context& c = ctx->c;
    API_ARG(&c, out_count && (host_dst || capacity == 0), "out_count / host_dst is NULL");
    API_ARG(&c, which <= 1u, "which must be 0 (Power_RIS tiles) or 1 (ReGIR cells)");
    return download_counted(c, which ? c.diCells.data() : c.diTiles.data(), which ? c.diCellCount : c.diTileCount, 1u, host_dst, capacity, out_count);
}

int pt_di_reset_history(PtContext* ctx)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    ctx->c.diHistoryValid = false;
    return PT_OK;
}

int pt_di_download_reservoirs(PtContext* ctx, PtDIReservoir* host_dst, uint32_t capacity, uint32_t* out_count)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    Context& c = ctx->c;
    API_ARG(&c, out_count && (host_dst || capacity == 0), "out_count / host_dst is NULL");
    return download_counted(c, c.diResB.data(), c.diResCount, 1u, host_dst, capacity, out_count);
}


int pt_di_light_count(PtContext* ctx, uint32_t* out_count)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    Context& c = ctx->c;
    API_ARG(&c, out_count, "out_count is NULL");
    API_HIP(&c, hipSetDevice(c.device));
    SceneView sv; FrameView fv; memset(&sv, 0, sizeof sv); memset(&fv, 0, sizeof fv);
    int st = make_views(c, 1, 1, sv, fv, false);
    if (st != PT_OK) return st;
    API_HIP(&c, ensure_light_list(c, sv));
    *out_count = c.lightCount;
    return PT_OK;
}

int pt_di_download_lights(PtContext* ctx, PtTriangleLight* host_dst, uint32_t capacity, uint32_t* out_count)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    Context& c = ctx->c;
    API_ARG(&c, out_count && (host_dst || capacity == 0), "out_count / host_dst is NULL");
    return download_counted(c, c.lightRecords.data(), c.lightRecordCount, 1u, host_dst, capacity, out_count);
}

} // extern "C"
