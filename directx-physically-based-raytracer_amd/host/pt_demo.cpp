// pt_demo.cpp -- C++ host of the path: builds the BASELINE Cornell box, drives libptamd.so through the
// reference-shaped operators of ptamd.hpp (GBufferGeneration / Raytracing / RaytracingHelpers), times it and
// optionally dumps the radiance for the parity test (tests/test_host_cpp.py compares it with the oracle).
//
//   pt_demo [--width W] [--height H] [--spp S] [--bounces B] [--frames N] [--out file.bin] [--ranks R] [--di] [--di-samples N] [--di-brdf-samples N [--di-brdf-cutoff C]] [--restir [--restir-pairwise] [--restir-visibility [--restir-raytraced]]] [--sharc]
//           [--light-sampling cdf|uniform|power_ris|regir [--regir-layout grid|onion]] [--di-pdf-mipmap]
//           [--post] [--no-bloom] [--bloom-strength S] [--tone-map saturate|reinhard|aces] [--exposure E]
//           [--hdr [--paper-white N] [--color-rotation hdtv_to_uhdtv|dci_p3_d65_to_uhdtv|hdtv_to_dci_p3_d65]]
//           [--nrd relax|reblur [--denoise [--denoise-frames-max N] [--denoise-iterations K]]] [--out-radiance file.bin]
//           [--upscale native|quality|balanced|performance|ultra [--output-size WxH] [--out-upscaled file.bin]]
//           [--reconstruct native|quality|balanced|performance|ultra --output-size WxH [--reconstruct-iterations K] [--out-reconstructed file.bin]]
//           [--frame-generation [--fg-phase PHI] [--out-generated file.bin] [--png-generated file.png]] [--camera-start X] [--camera-step DX]
//           [--sharpen [S] [--out-sharpened file.bin]]
//           [--png file.png] [--out-display file.bin] [--scene descriptor.json [--anim-time T [--anim-step DT]]] [--dump-scene file.bin]
//
// --anim-time T (with --scene): the animated render objects of the descriptor (RenderObjects[].Animation) are posed at T seconds of their selected
// clip before every frame -- on the device: AnimationCollection::Evaluate, skinning from the joint matrices it leaves, the refit of the skinned
// mesh nodes and the top level over the posed instances (Scene::Tick / Refresh / SkinSkeletalMeshes / CreateAccelerationStructures,
// Scene.ixx:174-188); --anim-step DT advances every clock by DT (Animation::Tick: it wraps at the clip's duration) between the timed frames.
//
// --di: the direct-lighting pass between the G-buffer and the path tracer (App.cpp:1234-1308), LocalLightSamples = --di-samples (default 8);
// --di-brdf-samples N adds N BRDF-sampled candidates per pixel, weighted by MIS against the light candidates (--di-brdf-cutoff C bounds their rays);
// the path tracer then runs with IsDIEnabled (with Bounces 0 the DI pass is the last render pass and adds to Radiance).
// --restir (with --di): temporal + spatial reservoir reuse at MyAppData's defaults; the Previous* G-buffer is swapped in before every
// frame after the first (App.cpp:629-634). Unsharded only.
// --restir-visibility (with --restir): visibility in the reservoirs at the RTXDI SDK's defaults (initial visibility, final-visibility reuse
// over 4 frames / 16 pixels); --restir-raytraced (with it): Raytraced bias correction in both passes.
// --restir-pairwise (with --restir): Pairwise bias correction in both passes (BiasCorrectionMode::Pairwise) instead of Basic; not
// together with --restir-raytraced.
// --light-sampling (with --di): how the DI pass draws its candidates (ReSTIRDI.InitialSampling.LocalLight.Mode; default cdf, the power
// prefix sum); ReGIR at MyAppData's cell size 1 and 8 build samples. --regir-layout (with --light-sampling regir): the layout of the
// ReGIR cells, the Grid (default) or the Onion the reference compiles.
// --di-pdf-mipmap (with --di): the DI pass builds the local-light PDF texture and its mip chain every frame (App::PrepareReSTIRDI), and
// power_ris / regir descend the chain for their light tiles instead of the power prefix sum; the JSON line then carries "di_pdf_mipmap": true.
//
// --post: the post-processing chain after every frame (App::PostProcessGraphics, App.cpp:1506-1571: Bloom + Merge, ToneMap, CopyTexture)
// at MyAppData's defaults (bloom 0.05, ACES filmic, exposure 0, SDR) unless the flags above change them; --png writes the last frame's
// Display8 as an RGB PNG (SDR only), --out-display its BackBuffer (R10G10B10A2_UNORM words). Both imply --post. With --ranks the chain
// runs on rank 0, on the gathered frame.
//
// --nrd relax|reblur: the frame is rendered with that Denoiser value (the G-buffer pass then writes the albedos, App.cpp:1223, and the path tracer the
// NRD-facing Diffuse / Specular), and App::ProcessNRD (App.cpp:1595-1688) runs after it and before --post: the NRD composition pass packs the pair,
// the denoiser -- the identity unless --denoise is given -- leaves it as it is, and the pass composes it into Radiance. With --ranks every rank
// runs the two passes on its own rows, before the gather. --out-radiance writes the last frame's Radiance (R16G16B16A16_FLOAT, the whole frame).
// --denoise (with --nrd relax, one unsharded process): the library's own denoiser (ptamd.hpp Denoiser: temporal accumulation, variance,
// a-trous) runs between the pack and the compose instead of the identity, at its defaults unless --denoise-frames-max (MaxAccumulatedFrames)
// or --denoise-iterations (AtrousIterations) change them. The timed frames are then one temporal sequence: they carry FrameIndex 0 .. N - 1
// in that order, and the history starts empty behind the warm-up frame. ReBLUR's packing is refused.
//
// --upscale MODE (one unsharded process): the frame is rendered at the render size of that super-resolution mode for the output size
// (--output-size WxH, else --width x --height; Upscaler::RenderSize) and the library's temporal upscaler (ptamd.hpp Upscaler) brings it to the
// output size after the NRD block and before --post, which then runs at the output size on the upscaled frame (--png / --out-display are
// output-size images). The camera keeps the output's aspect and carries the Halton jitter of the frame (Upscaler::Jitter). The timed
// frames are one temporal sequence: FrameIndex and the jitter index count 0 .. N - 1, and the history starts empty behind the warm-up
// frame. --out-upscaled writes the last frame's upscaled colour (R16G16B16A16_FLOAT at the output size). Composes with --nrd relax --denoise.
//
// --reconstruct MODE --output-size WxH (one unsharded process): the reference's default chain. The frame is rendered with Denoiser =
// DLSSRayReconstruction (the G-buffer pass then writes the albedos, Radiance stays the noisy sum) at the render size of that mode, jittered
// like --upscale, and the library's denoising upscaler (ptamd.hpp Reconstruction) brings it to the output size where the reference calls
// ProcessDLSSRayReconstruction (App.cpp:1513-1523), ahead of --post. --reconstruct-iterations K: its a-trous iterations (0..8, default 5).
// --out-reconstructed writes the last frame's Color (R16G16B16A16_FLOAT at the output size). Refused together with --upscale or --nrd (the
// pass is both steps); composes with --sharc, --di --restir, --post, --frames.
// --frame-generation (one unsharded process, needs --post and --frames 2 or more): the library's own frame interpolator (ptamd.hpp
// FrameGeneration; not a port of DLSS-G or FSR 3) runs behind the post chain of every frame, where the reference tags DLSS-G's inputs
// (App.cpp:1564-1566), on the post chain's Color, the frame's LinearDepth and MotionVector and its jitter. --fg-phase PHI: the phase between
// the two frames (default 0.5). --out-generated writes the frame generated between the last two rendered ones (R16G16B16A16_FLOAT at the
// output size), --png-generated its 8-bit form as an RGB PNG. Composes with --upscale, --reconstruct, --nrd ... --denoise. On a sequence
// that does not move the generated frame is the blend of the two.
// --sharpen [S]: the library's own adaptive sharpener (ptamd.hpp Sharpening; not a port of NVIDIA Image Scaling) runs where the reference
// runs ProcessNIS (App.cpp:1544-1548): behind --upscale / --reconstruct when given, else behind the frame (rank 0 of a sharded run, on the
// gathered frame), at the size --post runs at and ahead of it; --post then reads its output. S: Sharpness in [0, 1], default 0.5 (the
// reference's NIS.Sharpness). --out-sharpened writes the last frame's Sharpened (R16G16B16A16_FLOAT at that size). Composes with
// --upscale, --reconstruct, --nrd, --post and --frame-generation.
// --camera-start X --camera-step DX (one unsharded process): timed frame f is rendered from the scene's camera moved by X + f DX along world
// x, with the pose of frame f - 1 in the camera's Previous* members (the motion vectors follow); the warm-up frame stands at X.
//
// --ranks R: one process per GPU. The parent (which never touches a GPU) starts R children `--rank r --world R --id-file F`; rank 0
// makes the RCCL unique id and leaves it in F, the others pick it up; every rank renders its 16-row bands (BandSharding) and rank 0
// assembles the frame with pt_gather_bands (grouped ncclSend / ncclRecv over xGMI) -- the timed loop includes the gather. R may be 1
// (the N > 1 code path on a one-GPU box); R > the number of visible GPUs is refused (RCCL wants one device per rank).
//
// The scene construction mirrors scenes.py:cornell_box(variant="ggx") value for value (same double-precision
// expressions), so both hosts feed the library identical bytes. Build: make -C ../csrc ../pt_demo (hipcc, host code).
#include <hip/hip_runtime.h>
#include <signal.h>
#include <sys/wait.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <chrono>
#include <thread>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "ptamd.hpp"
#include "pt_png.hpp"
#include "pt_ingest.hpp"

using namespace ptamd;

#define HIP_OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(2); } } while (0)

struct Vertex {                    // VertexPositionNormalTangentTexture, Source/Vertex.ixx:38-50
    float Position[3];
    int16_t Normal[3], Tangent[3];
    uint16_t TexCoord[2][2];
};
static_assert(sizeof(Vertex) == 32, "layout");

static int16_t snorm16(double v)   // MathLib float2_to_snorm_16_16 (host side, Source/Vertex.ixx:17-22)
{
    v = std::fmin(std::fmax(v, -1.0), 1.0) * 32767.0;
    return (int16_t)(v >= 0 ? std::floor(v + 0.5) : std::ceil(v - 0.5));
}

struct HostMesh { std::vector<Vertex> vertices; std::vector<uint16_t> indices; PtMaterial material; };

static PtMaterial make_material(float r, float g, float b, float er = 0, float eg = 0, float eb = 0, float strength = 1, float metallic = 0,
                                float roughness = 0.5f, float ior = 1.5f, float transmission = 0)
{
    PtMaterial m{};                // Material() defaults, Source/Material.ixx:13-19
    m.BaseColor[0] = r; m.BaseColor[1] = g; m.BaseColor[2] = b; m.BaseColor[3] = 1;
    m.EmissiveStrength = strength; m.EmissiveColor[0] = er; m.EmissiveColor[1] = eg; m.EmissiveColor[2] = eb;
    m.Metallic = metallic; m.Roughness = roughness; m.IOR = ior; m.Transmission = transmission;
    m.AlphaMode = 0; m.AlphaCutoff = 0.5f;
    return m;
}

static HostMesh quad(const double p[4][3], const double n[3], const PtMaterial& mat)
{
    HostMesh m; m.material = mat;
    for (int i = 0; i < 4; i++) {
        Vertex v{};
        for (int k = 0; k < 3; k++) { v.Position[k] = (float)p[i][k]; v.Normal[k] = snorm16(n[k]); }
        m.vertices.push_back(v);
    }
    m.indices = { 0, 1, 2, 0, 2, 3 };
    return m;
}

static HostMesh box(const PtMaterial& mat)   // unit cube, 24 vertices with face normals (scenes.py:box_mesh)
{
    HostMesh m; m.material = mat;
    for (int axis = 0; axis < 3; axis++)
        for (int si = 0; si < 2; si++) {
            const double sgn = si ? 1.0 : -1.0;
            const int a = (axis + 1) % 3, b = (axis + 2) % 3;
            const int sa[4] = { -1, 1, 1, -1 }, sb[4] = { -1, -1, 1, 1 };
            double corners[4][3];
            for (int c = 0; c < 4; c++) { corners[c][axis] = 0.5 * sgn; corners[c][a] = 0.5 * sa[c]; corners[c][b] = 0.5 * sb[c]; }
            const uint16_t base = (uint16_t)m.vertices.size();
            for (int c = 0; c < 4; c++) {
                const double* p = corners[sgn < 0 ? 3 - c : c];
                Vertex v{};
                for (int k = 0; k < 3; k++) { v.Position[k] = (float)p[k]; v.Normal[k] = snorm16(k == axis ? sgn : 0.0); }
                m.vertices.push_back(v);
            }
            const uint16_t q[6] = { 0, 1, 2, 0, 2, 3 };
            for (uint16_t i : q) m.indices.push_back((uint16_t)(base + i));
        }
    return m;
}

static void trs(float out[12], double tx, double ty, double tz, double yawDeg, double sx, double sy, double sz)
{   // scenes.py:trs with pitch = 0: T * R_y(yaw) * S, column-vector 3x4
    const double a = yawDeg * (M_PI / 180.0), cy = std::cos(a), sn = std::sin(a);
    const double ry[3][3] = { { cy, 0, sn }, { 0, 1, 0 }, { -sn, 0, cy } };
    const double s[3] = { sx, sy, sz }, t[3] = { tx, ty, tz };
    for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) out[4 * i + j] = (float)(ry[i][j] * s[j]); out[4 * i + 3] = (float)t[i]; }
}

template <typename T> static T* upload(const std::vector<T>& v)
{
    T* d = nullptr;
    HIP_OK(hipMalloc((void**)&d, v.size() * sizeof(T) + 16));
    HIP_OK(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return d;
}

// What the host hands the library, whichever way it came about (built in code below, or loaded by pt_ingest.hpp): mesh nodes (one bottom level
// each, one geometry per mesh), instances of them, a camera and the environment.
struct HostGeometry { std::vector<uint8_t> vertices; uint32_t vertexCount = 0; std::vector<uint8_t> indices; uint32_t indexCount = 0, indexStride = 2;
                      bool hasNormals = true, hasTangents = false, hasUV[2] = { false, false }; PtMaterial material{};
                      std::shared_ptr<ingest::Texture> textures[7]; uint32_t texCoord[7] = { 0, 0, 0, 0, 0, 0, 0 };       // slots in the order of Material.ixx:22-33
                      std::vector<uint8_t> skeletal; };                  // a skinned mesh: its 48-byte skeletal vertices (vertexCount of them), else empty
struct HostNode { std::vector<HostGeometry> meshes; };
struct HostObject { uint32_t node = 0; float transform[12]; bool visible = true; };
struct HostScene {
    std::vector<HostNode> nodes; std::vector<HostObject> objects;
    double cameraPosition[3] = { 0, 0, 0 }, cameraForward[3] = { 0, 0, 1 }, cameraUp[3] = { 0, 1, 0 };
    float envColor[4] = { 0, 0, 0, 1 }, envTransform[12] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0 };
    std::vector<ingest::AnimatedObject> animations;                  // render objects with an animation bound, rigs resolved to indices
};

static HostGeometry to_geometry(const HostMesh& m)
{
    HostGeometry g;
    g.vertexCount = (uint32_t)m.vertices.size(); g.vertices.resize(m.vertices.size() * sizeof(Vertex)); memcpy(g.vertices.data(), m.vertices.data(), g.vertices.size());
    g.indexCount = (uint32_t)m.indices.size(); g.indices.resize(m.indices.size() * 2); memcpy(g.indices.data(), m.indices.data(), g.indices.size());
    g.material = m.material;
    return g;
}

// scenes.py:cornell_box, variant "ggx": one mesh node per object, camera at the front opening looking +Z
static HostScene cornell_scene()
{
    HostScene sc;
    const PtMaterial white = make_material(0.73f, 0.73f, 0.73f), red = make_material(0.65f, 0.05f, 0.05f), green = make_material(0.12f, 0.45f, 0.15f);
    const double floorP[4][3] = { { -1, -1, -1 }, { -1, -1, 1 }, { 1, -1, 1 }, { 1, -1, -1 } }, up[3] = { 0, 1, 0 };
    const double ceilP[4][3] = { { -1, 1, -1 }, { 1, 1, -1 }, { 1, 1, 1 }, { -1, 1, 1 } }, down[3] = { 0, -1, 0 };
    const double backP[4][3] = { { -1, -1, 1 }, { -1, 1, 1 }, { 1, 1, 1 }, { 1, -1, 1 } }, toCam[3] = { 0, 0, -1 };
    const double leftP[4][3] = { { -1, -1, -1 }, { -1, 1, -1 }, { -1, 1, 1 }, { -1, -1, 1 } }, px[3] = { 1, 0, 0 };
    const double rightP[4][3] = { { 1, -1, -1 }, { 1, -1, 1 }, { 1, 1, 1 }, { 1, 1, -1 } }, nx[3] = { -1, 0, 0 };
    const double lightP[4][3] = { { -0.25, 0, -0.25 }, { 0.25, 0, -0.25 }, { 0.25, 0, 0.25 }, { -0.25, 0, 0.25 } };
    const std::vector<HostMesh> meshes = {
        quad(floorP, up, white), quad(ceilP, down, white), quad(backP, toCam, white), quad(leftP, px, red), quad(rightP, nx, green),
        quad(lightP, down, make_material(0.78f, 0.78f, 0.78f, 1, 1, 1, 15.0f)),
        box(make_material(0.95f, 0.93f, 0.88f, 0, 0, 0, 1, 1.0f, 0.05f)), box(make_material(0.73f, 0.73f, 0.73f, 0, 0, 0, 1, 0, 0.2f)) };
    float xf[8][12];
    for (int i = 0; i < 5; i++) trs(xf[i], 0, 0, 0, 0, 1, 1, 1);
    trs(xf[5], 0, 0.998, 0.1, 0, 1, 1, 1);
    trs(xf[6], -0.35, -0.4, 0.35, -18.0, 0.6, 1.2, 0.6);
    trs(xf[7], 0.35, -0.7, -0.25, 15.0, 0.6, 0.6, 0.6);
    for (size_t i = 0; i < meshes.size(); i++) {
        HostNode n; n.meshes.push_back(to_geometry(meshes[i])); sc.nodes.push_back(std::move(n));
        HostObject o; o.node = (uint32_t)i; memcpy(o.transform, xf[i], 48); sc.objects.push_back(o);
    }
    sc.cameraPosition[2] = -1.95;
    return sc;
}

// a scene descriptor in the reference's schema (Source/MyScene.ixx:33-90) with its glTF models, through host/pt_ingest.hpp.
// Camera: App::ResetCamera = CameraController::SetPosition / SetRotation (Source/Camera.ixx:84-97), default lens.
static HostScene ingested_scene(const std::string& path)
{
    const ingest::Scene in = ingest::load_scene(path);
    HostScene sc;
    for (auto& node : in.Nodes) {
        HostNode n;
        for (const ingest::MeshData& md : node->Meshes) {
            HostGeometry g;
            g.vertexCount = (uint32_t)md.Vertices.size(); g.vertices.resize(md.Vertices.size() * sizeof(ingest::Vertex)); memcpy(g.vertices.data(), md.Vertices.data(), g.vertices.size());
            g.indices = md.Indices; g.indexCount = md.IndexCount; g.indexStride = md.IndexStride;
            g.hasNormals = md.HasNormals; g.hasTangents = md.HasTangents; g.hasUV[0] = md.HasUV[0]; g.hasUV[1] = md.HasUV[1];
            g.material = md.HasMaterial ? md.Material : ingest::default_material();            // App.cpp:1044: Material() when a mesh names none
            for (int k = 0; k < 7; k++) { g.textures[k] = md.Textures[k]; g.texCoord[k] = md.TextureCoordinateIndex[k]; }
            g.skeletal.resize(md.SkeletalVertices.size() * sizeof(ingest::SkeletalVertex)); if (!g.skeletal.empty()) memcpy(g.skeletal.data(), md.SkeletalVertices.data(), g.skeletal.size());
            for (const std::string& slot : md.SkippedTextures) fprintf(stderr, "pt_demo: %s texture of a material not loaded (this host decodes 8-bit PNG and reads BC1 / BC3 / BC4 / BC5 or RGBA8 DDS only)\n", slot.c_str());
            n.meshes.push_back(std::move(g));
        }
        sc.nodes.push_back(std::move(n));
    }
    for (const ingest::RenderObject& ro : in.Objects) { HostObject o; o.node = ro.Node; memcpy(o.transform, ro.Transform, 48); o.visible = ro.IsVisible; sc.objects.push_back(o); }
    const ingest::M4& r = in.CameraRotation;                         // forward = (0,0,1,0) R, right = (1,0,0,0) R, up = forward x right (ingest.py camera_from_desc)
    const double fwd[3] = { r.m[2][0], r.m[2][1], r.m[2][2] }, right[3] = { r.m[0][0], r.m[0][1], r.m[0][2] };
    for (int k = 0; k < 3; k++) { sc.cameraPosition[k] = in.CameraPosition[k]; sc.cameraForward[k] = fwd[k]; }
    sc.cameraUp[0] = fwd[1] * right[2] - fwd[2] * right[1]; sc.cameraUp[1] = fwd[2] * right[0] - fwd[0] * right[2]; sc.cameraUp[2] = fwd[0] * right[1] - fwd[1] * right[0];
    memcpy(sc.envColor, in.EnvironmentLightColor, 16); memcpy(sc.envTransform, in.EnvironmentLightTransform, 48);
    sc.animations = in.Animations;
    return sc;
}

// scenes.py:make_camera (hfov 90, near 0.01, far inf): XMMatrixLookToLH + SetupByHalfFovxInf, row-vector convention
static PtCamera make_camera(const HostScene& sc, double aspect, const double* position = nullptr)
{
    auto norm = [](double v[3]) { const double l = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); v[0] /= l; v[1] /= l; v[2] /= l; };
    auto cross = [](const double a[3], const double b[3], double o[3]) { o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0]; };
    auto dot = [](const double a[3], const double b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; };
    double f[3] = { sc.cameraForward[0], sc.cameraForward[1], sc.cameraForward[2] }, r[3], u[3];
    norm(f); cross(sc.cameraUp, f, r); norm(r); cross(f, r, u);
    const double* pos = position ? position : sc.cameraPosition;
    const double rightLen = std::tan((90.0 * (M_PI / 180.0)) / 2), upLen = rightLen / aspect, nearD = 0.01;
    PtCamera cam{};
    cam.IsNormalizedDepthReversed = 1;
    for (int k = 0; k < 3; k++) {
        cam.Position[k] = cam.PreviousPosition[k] = (float)pos[k];
        cam.RightDirection[k] = (float)(r[k] * rightLen); cam.UpDirection[k] = (float)(u[k] * upLen); cam.ForwardDirection[k] = (float)f[k];
    }
    cam.NearDepth = (float)nearD; cam.FarDepth = std::numeric_limits<float>::infinity();
    double w2v[4][4] = {}, v2p[4][4] = {}, w2p[4][4] = {};
    for (int k = 0; k < 3; k++) { w2v[k][0] = r[k]; w2v[k][1] = u[k]; w2v[k][2] = f[k]; }
    w2v[3][0] = -dot(pos, r); w2v[3][1] = -dot(pos, u); w2v[3][2] = -dot(pos, f); w2v[3][3] = 1;
    v2p[0][0] = 1 / rightLen; v2p[1][1] = aspect / rightLen; v2p[2][3] = 1; v2p[3][2] = nearD;
    for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) for (int k = 0; k < 4; k++) w2p[i][j] += w2v[i][k] * v2p[k][j];
    for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) {
        cam.WorldToProjection[4 * i + j] = cam.PreviousWorldToProjection[4 * i + j] = (float)w2p[i][j];
        cam.PreviousWorldToView[4 * i + j] = (float)w2v[i][j]; cam.PreviousViewToProjection[4 * i + j] = (float)v2p[i][j];
    }
    // ProjectionToView = inverse(ViewToProjection) (its infinite-far form inverts in closed form), ViewToWorld = rows Right, Up, Forward,
    // Position: what the direct-lighting pass reconstructs surface positions with (scenes.py:make_camera, Camera::ReconstructWorldPosition)
    double p2v[4][4] = {}, v2w[4][4] = {};
    p2v[0][0] = 1 / v2p[0][0]; p2v[1][1] = 1 / v2p[1][1]; p2v[2][3] = 1 / v2p[3][2]; p2v[3][2] = 1 / v2p[2][3];
    for (int k = 0; k < 3; k++) { v2w[0][k] = r[k]; v2w[1][k] = u[k]; v2w[2][k] = f[k]; v2w[3][k] = pos[k]; }
    v2w[3][3] = 1;
    for (int i = 0; i < 16; i++) {
        cam.ProjectionToView[i] = cam.PreviousProjectionToView[i] = (float)p2v[i / 4][i % 4];
        cam.ViewToWorld[i] = cam.PreviousViewToWorld[i] = (float)v2w[i / 4][i % 4];
    }
    return cam;
}

// the camera at `position` whose Previous* members are the camera at `previous`: a frame of a camera that moves (--camera-step)
static PtCamera make_moved_camera(const HostScene& sc, double aspect, const double* position, const double* previous)
{
    PtCamera cam = make_camera(sc, aspect, position);
    const PtCamera prev = make_camera(sc, aspect, previous);
    memcpy(cam.PreviousPosition, prev.Position, sizeof cam.PreviousPosition);
    memcpy(cam.PreviousWorldToProjection, prev.WorldToProjection, sizeof cam.PreviousWorldToProjection);
    memcpy(cam.PreviousProjectionToView, prev.ProjectionToView, sizeof cam.PreviousProjectionToView);
    memcpy(cam.PreviousViewToWorld, prev.ViewToWorld, sizeof cam.PreviousViewToWorld);
    memcpy(cam.PreviousWorldToView, prev.PreviousWorldToView, sizeof cam.PreviousWorldToView);
    memcpy(cam.PreviousViewToProjection, prev.PreviousViewToProjection, sizeof cam.PreviousViewToProjection);
    return cam;
}

// --dump-scene: what would be handed to the library, byte for byte, without touching a GPU (tests/test_host_cpp.py compares it with the harness's ingest)
static int dump_scene(const HostScene& sc, const std::string& path)
{
    FILE* fp = fopen(path.c_str(), "wb");
    if (!fp) { fprintf(stderr, "cannot open %s\n", path.c_str()); return 3; }
    printf("{\"nodes\": [");
    for (size_t n = 0; n < sc.nodes.size(); n++) {
        printf("%s[", n ? ", " : "");
        for (size_t m = 0; m < sc.nodes[n].meshes.size(); m++) {
            const HostGeometry& g = sc.nodes[n].meshes[m];
            printf("%s{\"vertices\": %u, \"indices\": %u, \"index_stride\": %u, \"has_normals\": %d, \"has_tangents\": %d, \"has_uv\": [%d, %d], \"textures\": [", m ? ", " : "",
                   g.vertexCount, g.indexCount, g.indexStride, g.hasNormals, g.hasTangents, g.hasUV[0], g.hasUV[1]);
            fwrite(g.vertices.data(), 1, g.vertices.size(), fp); fwrite(g.indices.data(), 1, g.indices.size(), fp); fwrite(&g.material, sizeof(PtMaterial), 1, fp);
            bool firstTex = true;
            for (int k = 0; k < 7; k++) if (g.textures[k]) {              // slot, size, sRGB, coordinate set; the texels follow the material in the file
                const ingest::Texture& t = *g.textures[k];                // a block-compressed texture: a sixth entry, its PtFormat, and the block bytes in the file
                printf("%s[%d, %u, %u, %d, %u", firstTex ? "" : ", ", k, t.Texels.Width, t.Texels.Height, t.SRGB ? 1 : 0, g.texCoord[k]);
                if (t.IsBlockCompressed()) { printf(", %u]", (unsigned)t.Format()); fwrite(t.Blocks.data(), 1, t.Blocks.size(), fp); }
                else { printf("]"); fwrite(t.Texels.RGBA.data(), 1, t.Texels.RGBA.size(), fp); }
                firstTex = false;
            }
            printf("]}");
        }
        printf("]");
    }
    printf("], \"objects\": [");
    for (size_t i = 0; i < sc.objects.size(); i++) { printf("%s{\"node\": %u, \"visible\": %d}", i ? ", " : "", sc.objects[i].node, sc.objects[i].visible ? 1 : 0); fwrite(sc.objects[i].transform, 4, 12, fp); }
    // the resolved rigs, behind everything else in the file: per animated object the arrays of pt_anim_create_rig (parents, rest TRS, durations,
    // channels, key times, key values) and of pt_anim_create_object (transform, binding nodes / instances / globals, then per skin its joint nodes
    // and inverse bind matrices); then the skeletal vertices of every skinned mesh, in node order
    printf("], \"animations\": [");
    fwrite(sc.envColor, 4, 4, fp); fwrite(sc.envTransform, 4, 12, fp);
    const PtCamera cam = make_camera(sc, 16.0 / 9.0);
    fwrite(&cam, sizeof cam, 1, fp);
    auto put = [&](const auto& v) { if (!v.empty()) fwrite(v.data(), sizeof v[0], v.size(), fp); };
    auto list = [&](const auto& v) { printf("["); for (size_t k = 0; k < v.size(); k++) printf("%s%lld", k ? ", " : "", (long long)v[k]); printf("]"); };
    for (size_t a = 0; a < sc.animations.size(); a++) {
        const ingest::AnimatedObject& ao = sc.animations[a]; const ingest::Rig& r = *ao.Animation;
        put(r.Parents); put(r.Rest); put(r.Durations); put(r.Channels); put(r.KeyTimes); put(r.KeyValues);
        fwrite(ao.Transform, 4, 16, fp); put(ao.BindingNodes); put(ao.BindingInstances); put(ao.BindingGlobals);
        for (const auto& sk : ao.Skins) { put(sk.JointNodes); put(sk.InverseBinds); }
        std::vector<uint32_t> keyCounts;
        for (size_t k = 1; k < r.Channels.size(); k += 2) keyCounts.push_back(r.Channels[k]);
        printf("%s{\"nodes\": %zu, \"clips\": %zu, \"keys\": %zu, \"parents\": ", a ? ", " : "", r.Parents.size(), r.Durations.size(), r.KeyTimes.size()); list(r.Parents);
        printf(", \"key_counts\": "); list(keyCounts);
        printf(", \"binding_nodes\": "); list(ao.BindingNodes); printf(", \"binding_instances\": "); list(ao.BindingInstances);
        printf(", \"skins\": [");
        for (size_t k = 0; k < ao.Skins.size(); k++) { printf("%s{\"mesh_node\": %u, \"scene_node\": %u, \"joints\": ", k ? ", " : "", ao.Skins[k].MeshNode, ao.Skins[k].SceneNode); list(ao.Skins[k].JointNodes); printf("}"); }
        printf("]}");
    }
    printf("], \"skeletal\": [");
    bool firstSkeletal = true;
    for (size_t n = 0; n < sc.nodes.size(); n++) for (size_t m = 0; m < sc.nodes[n].meshes.size(); m++) if (!sc.nodes[n].meshes[m].skeletal.empty()) {
        printf("%s[%zu, %zu]", firstSkeletal ? "" : ", ", n, m); firstSkeletal = false;
        put(sc.nodes[n].meshes[m].skeletal);
    }
    printf("]}\n");
    fclose(fp);
    return 0;
}

// --ranks R: start one child per rank and wait for them (no GPU call has been made in this process, and none will be).
// The unique id travels through a file in a directory of our own (mkdtemp: mode 0700, unpredictable name). The first rank that fails
// ends the run: the others would wait for it inside ncclCommInitRank or a grouped receive for ever, so they are killed.
static int launch_ranks(int argc, char** argv, uint32_t ranks)
{
    char dirTemplate[] = "/tmp/pt_demo_XXXXXX";
    if (!mkdtemp(dirTemplate)) { perror("mkdtemp"); return 2; }
    const std::string dir = dirTemplate, idFile = dir + "/id";
    std::vector<pid_t> pids;
    int rc = 0;
    for (uint32_t r = 0; r < ranks && rc == 0; r++) {
        const pid_t pid = fork();
        if (pid < 0) { perror("fork"); rc = 2; break; }
        if (pid == 0) {
            std::vector<std::string> args(argv, argv + argc);
            for (const char* extra : { "--rank", "", "--world", "", "--id-file", "" }) args.push_back(extra);
            args[args.size() - 5] = std::to_string(r); args[args.size() - 3] = std::to_string(ranks); args[args.size() - 1] = idFile;
            std::vector<char*> cargs;
            for (auto& a : args) cargs.push_back(a.data());
            cargs.push_back(nullptr);
            execv("/proc/self/exe", cargs.data());
            perror("execv"); _exit(127);
        }
        pids.push_back(pid);
    }
    size_t left = pids.size();
    while (left) {
        int st = 0;
        const pid_t p = waitpid(-1, &st, 0);
        if (p < 0) { if (errno == EINTR) continue; break; }
        auto it = std::find(pids.begin(), pids.end(), p);
        if (it == pids.end()) continue;
        *it = -1; left--;
        const int code = WIFEXITED(st) ? WEXITSTATUS(st) : 2;
        if (code != 0 && rc == 0) {
            rc = code;
            for (pid_t q : pids) if (q > 0) kill(q, SIGTERM);                     // exactly the children started above
        }
    }
    unlink((idFile + ".tmp").c_str()); unlink(idFile.c_str()); rmdir(dir.c_str());
    return rc;
}

static std::vector<uint8_t> exchange_unique_id(uint32_t rank, const std::string& idFile)
{
    std::vector<uint8_t> id(PT_COMM_ID_BYTES);
    if (rank == 0) {
        id = BandSharding::UniqueId();
        const std::string tmp = idFile + ".tmp";
        FILE* fp = fopen(tmp.c_str(), "wb");
        if (!fp || fwrite(id.data(), 1, id.size(), fp) != id.size()) throw std::runtime_error("cannot write " + tmp);
        fclose(fp);
        if (rename(tmp.c_str(), idFile.c_str()) != 0) throw std::runtime_error("cannot publish " + idFile);
        return id;
    }
    for (int tries = 0; tries < 1200; tries++) {                    // rank 0 publishes with an atomic rename: a file that exists is complete
        if (FILE* fp = fopen(idFile.c_str(), "rb")) {
            const size_t n = fread(id.data(), 1, id.size(), fp);
            fclose(fp);
            if (n == id.size()) return id;
        }
        std::this_thread::sleep_for(std::chrono::milliseconds(50));
    }
    throw std::runtime_error("rank 0 never published the RCCL unique id");
}

int main(int argc, char** argv)
{
    uint32_t W = 1920, H = 1080, spp = 4, bounces = 8, frames = 10, ranks = 0, rank = 0, world = 1;
    uint32_t diSamples = 8, diBrdfSamples = 0; float diBrdfCutoff = 0.0f; bool di = false, diPdfMipmap = false, restir = false, restirVisibility = false, restirRaytraced = false, restirPairwise = false;
    bool useSharc = false; uint32_t sharcDownscale = 4; float sceneScale = 50.0f;   // --sharc [--sharc-downscale N --scene-scale S]: frames through the radiance cache
    std::string out, idFile, scenePath, dumpPath, lightSampling = "cdf", regirLayout = "grid";
    bool post = false, bloom = true, hdr = false; float bloomStrength = 0.05f, exposure = 0.0f, paperWhite = 200.0f;
    std::string toneMap = "aces", colorRotation = "hdtv_to_uhdtv", pngPath, displayPath;
    bool animate = false; double animTime = 0.0, animStep = 0.0;
    std::string nrd, radiancePath;
    bool denoise = false; uint32_t denoiseFramesMax = 30, denoiseIterations = 5;
    std::string upscale, outputSize, upscaledPath;
    std::string reconstruct, reconstructedPath; int reconstructIterations = -1;
    bool frameGeneration = false; float fgPhase = 0.5f; std::string generatedPath, generatedPngPath;
    bool cameraMoves = false; double cameraStart = 0.0, cameraStep = 0.0;
    bool sharpen = false; float sharpness = 0.5f; std::string sharpenedPath;
    for (int i = 1; i < argc; i++) {
        std::string k = argv[i];
        if (k == "--di") { di = true; continue; }                  // the flags without a value
        if (k == "--di-pdf-mipmap") { diPdfMipmap = true; continue; }
        if (k == "--restir") { restir = true; continue; }
        if (k == "--restir-visibility") { restirVisibility = true; continue; }
        if (k == "--restir-raytraced") { restirRaytraced = true; continue; }
        if (k == "--restir-pairwise") { restirPairwise = true; continue; }
        if (k == "--sharc") { useSharc = true; continue; }
        if (k == "--post") { post = true; continue; }
        if (k == "--no-bloom") { bloom = false; continue; }
        if (k == "--hdr") { hdr = true; continue; }
        if (k == "--denoise") { denoise = true; continue; }
        if (k == "--frame-generation") { frameGeneration = true; continue; }
        if (k == "--sharpen") {                                    // its value is optional: a following word that is not a flag
            sharpen = true;
            if (i + 1 < argc && strncmp(argv[i + 1], "--", 2) != 0) sharpness = (float)atof(argv[++i]);
            continue;
        }
        if (i + 1 >= argc) break;
        const char* v = argv[++i];
        if (k == "--width") W = atoi(v); else if (k == "--height") H = atoi(v);
        else if (k == "--spp") spp = atoi(v); else if (k == "--bounces") bounces = atoi(v);
        else if (k == "--frames") frames = atoi(v); else if (k == "--out") out = v;
        else if (k == "--ranks") ranks = atoi(v); else if (k == "--rank") rank = atoi(v);
        else if (k == "--world") world = atoi(v); else if (k == "--id-file") idFile = v;
        else if (k == "--di-samples") diSamples = atoi(v);
        else if (k == "--di-brdf-samples") diBrdfSamples = atoi(v); else if (k == "--di-brdf-cutoff") diBrdfCutoff = (float)atof(v);
        else if (k == "--sharc-downscale") sharcDownscale = atoi(v); else if (k == "--scene-scale") sceneScale = (float)atof(v);
        else if (k == "--light-sampling") lightSampling = v; else if (k == "--regir-layout") regirLayout = v;
        else if (k == "--scene") scenePath = v; else if (k == "--dump-scene") dumpPath = v;
        else if (k == "--bloom-strength") bloomStrength = (float)atof(v); else if (k == "--tone-map") toneMap = v;
        else if (k == "--exposure") exposure = (float)atof(v); else if (k == "--paper-white") paperWhite = (float)atof(v);
        else if (k == "--color-rotation") colorRotation = v; else if (k == "--png") pngPath = v;
        else if (k == "--out-display") displayPath = v;
        else if (k == "--denoise-frames-max") denoiseFramesMax = atoi(v); else if (k == "--denoise-iterations") denoiseIterations = atoi(v);
        else if (k == "--nrd") nrd = v; else if (k == "--out-radiance") radiancePath = v;
        else if (k == "--upscale") upscale = v; else if (k == "--output-size") outputSize = v; else if (k == "--out-upscaled") upscaledPath = v;
        else if (k == "--reconstruct") reconstruct = v; else if (k == "--out-reconstructed") reconstructedPath = v;
        else if (k == "--reconstruct-iterations") reconstructIterations = atoi(v);
        else if (k == "--fg-phase") fgPhase = (float)atof(v); else if (k == "--out-generated") generatedPath = v; else if (k == "--png-generated") generatedPngPath = v;
        else if (k == "--out-sharpened") sharpenedPath = v;
        else if (k == "--camera-start") { cameraMoves = true; cameraStart = atof(v); } else if (k == "--camera-step") { cameraMoves = true; cameraStep = atof(v); }
        else if (k == "--anim-time") { animate = true; animTime = atof(v); } else if (k == "--anim-step") animStep = atof(v);
    }
    post = post || !pngPath.empty() || !displayPath.empty();
    const bool sharded = !idFile.empty();
    if (!dumpPath.empty()) {                                        // no GPU call on this path
        try { return dump_scene(scenePath.empty() ? cornell_scene() : ingested_scene(scenePath), dumpPath); }
        catch (const std::exception& e) { fprintf(stderr, "pt_demo: %s\n", e.what()); return 1; }
    }
    if (ranks && !sharded) return launch_ranks(argc, argv, ranks);
    try {
        // ---- --upscale: W x H becomes the render size of the mode for the output size
        // ---- --reconstruct: the same sizes and jitter, with the denoising upscaler in the upscaler's place and no NRD block
        const bool upscaling = !upscale.empty(), reconstructing = !reconstruct.empty(), resizing = upscaling || reconstructing;
        uint32_t outW = W, outH = H;
        if (reconstructing) {
            if (upscaling) throw std::invalid_argument("--reconstruct is the denoiser and the upscaler of its frame: drop --upscale");
            if (!nrd.empty() || denoise) throw std::invalid_argument("--reconstruct is the denoiser and the upscaler of its frame: drop --nrd / --denoise");
            if (sharded) throw std::invalid_argument("--reconstruct needs one unsharded process");
            if (outputSize.empty()) throw std::invalid_argument("--reconstruct needs --output-size WxH");
            if (reconstructIterations != -1 && (reconstructIterations < 0 || reconstructIterations > 8)) throw std::invalid_argument("--reconstruct-iterations: 0..8");
            if (reconstruct != "native" && reconstruct != "quality" && reconstruct != "balanced" && reconstruct != "performance" && reconstruct != "ultra")
                throw std::invalid_argument("--reconstruct: native, quality, balanced, performance or ultra");
            upscale = reconstruct;                                  // the mode names and the render sizes are the upscaler's
        } else if (reconstructIterations != -1 || !reconstructedPath.empty())
            throw std::invalid_argument("--reconstruct-iterations and --out-reconstructed need --reconstruct");
        if (resizing) {
            if (sharded) throw std::invalid_argument("--upscale needs one unsharded process");
            Upscaler::SuperResolutionMode mode;
            if (upscale == "native") mode = PT_SUPER_RESOLUTION_NATIVE; else if (upscale == "quality") mode = PT_SUPER_RESOLUTION_QUALITY;
            else if (upscale == "balanced") mode = PT_SUPER_RESOLUTION_BALANCED; else if (upscale == "performance") mode = PT_SUPER_RESOLUTION_PERFORMANCE;
            else if (upscale == "ultra") mode = PT_SUPER_RESOLUTION_ULTRA_PERFORMANCE;
            else throw std::invalid_argument("--upscale: native, quality, balanced, performance or ultra");
            if (!outputSize.empty() && sscanf(outputSize.c_str(), "%ux%u", &outW, &outH) != 2) throw std::invalid_argument("--output-size: WxH");
            const uint32_t output[2] = { outW, outH }; uint32_t render[2];
            Upscaler::RenderSize(mode, output, render);
            W = render[0]; H = render[1];
        } else if (!outputSize.empty() || !upscaledPath.empty()) throw std::invalid_argument("--output-size and --out-upscaled need --upscale");
        if (frameGeneration) {
            if (!post) throw std::invalid_argument("--frame-generation interpolates the tone-mapped Color: it needs --post");
            if (sharded) throw std::invalid_argument("--frame-generation needs one unsharded process");
            if (frames < 2) throw std::invalid_argument("--frame-generation needs --frames 2 or more: the first frame has no predecessor");
            if (hdr && !generatedPngPath.empty()) throw std::invalid_argument("--png-generated writes an SDR image: drop --hdr");
        } else if (fgPhase != 0.5f || !generatedPath.empty() || !generatedPngPath.empty())
            throw std::invalid_argument("--fg-phase, --out-generated and --png-generated need --frame-generation");
        if (!sharpen && !sharpenedPath.empty()) throw std::invalid_argument("--out-sharpened needs --sharpen");
        if (cameraMoves && sharded) throw std::invalid_argument("--camera-start / --camera-step need one unsharded process");
        int deviceCount = 0;
        HIP_OK(hipGetDeviceCount(&deviceCount));
        if ((int)world > deviceCount) { fprintf(stderr, "pt_demo: %u ranks need %u GPUs, %d visible\n", world, world, deviceCount); return 4; }
        HIP_OK(hipSetDevice((int)rank));
        hipStream_t stream; HIP_OK(hipStreamCreate(&stream));
        CommandList commandList((int)rank, stream);
        BandSharding sharding;
        if (sharded) sharding.Join(commandList, rank, world, exchange_unique_id(rank, idFile).data());
        const uint32_t localRows = sharding.LocalRows(H);

        // ---- scene: the Cornell box built in code (scenes.py:cornell_box, variant "ggx"), or --scene <descriptor.json> through pt_ingest.hpp
        const HostScene scene = scenePath.empty() ? cornell_scene() : ingested_scene(scenePath);

        // ---- buffers, descriptor heap, bottom levels (Scene::CreateAccelerationStructures: one per mesh node, one geometry per mesh)
        uint32_t heapSize = 0;
        std::map<const ingest::Texture*, uint32_t> textureDescriptor;        // one descriptor per texture, however many meshes share it
        for (const HostNode& nd : scene.nodes) {
            heapSize += 2 * (uint32_t)nd.meshes.size();
            for (const HostGeometry& hg : nd.meshes) for (auto& t : hg.textures) if (t && !textureDescriptor.count(t.get())) textureDescriptor[t.get()] = 0;
        }
        const uint32_t firstTextureDescriptor = heapSize;
        heapSize += (uint32_t)textureDescriptor.size();
        const uint32_t firstMotionDescriptor = heapSize;                     // one motion-vector buffer per skinned mesh (MeshDescriptors.MotionVectors)
        for (const HostNode& nd : scene.nodes) for (const HostGeometry& hg : nd.meshes) if (!hg.skeletal.empty()) heapSize++;
        ThrowIfFailed(commandList.Context, pt_heap_resize(commandList.Context, heapSize));
        {
            uint32_t next = firstTextureDescriptor;
            for (auto& kv : textureDescriptor) {                             // texel arrays as pt_heap_set_texture takes them (App.cpp:1052-1063 fills the descriptor indices)
                kv.second = next++;
                const ingest::Image& im = kv.first->Texels;                 // a DDS texture goes up as the blocks of its file, under its block format
                uint8_t* dt = upload(kv.first->IsBlockCompressed() ? kv.first->Blocks : im.RGBA);
                ThrowIfFailed(commandList.Context, pt_heap_set_texture(commandList.Context, kv.second, dt, im.Width, im.Height, kv.first->Format(), 0));
            }
        }
        struct GeometryOnDevice { uint32_t heapVertices, heapIndices, heapMotion; uint8_t* vertices; uint8_t* skeletal; uint8_t* motion; uint32_t vertexCount; };
        std::vector<std::vector<GeometryOnDevice>> onDevice(scene.nodes.size());
        std::vector<uint64_t> blas(scene.nodes.size());
        std::vector<std::vector<PtGeometryDesc>> nodeGeoms(scene.nodes.size());
        uint32_t heapNext = 0, motionNext = firstMotionDescriptor;
        for (size_t ni = 0; ni < scene.nodes.size(); ni++) {
            std::vector<PtGeometryDesc>& geoms = nodeGeoms[ni];
            bool skeletal = false;
            for (const HostGeometry& hg : scene.nodes[ni].meshes) {
                uint8_t* dv = upload(hg.vertices); uint8_t* di = upload(hg.indices);
                ThrowIfFailed(commandList.Context, pt_heap_set_buffer(commandList.Context, heapNext, dv, hg.vertices.size(), 0));
                ThrowIfFailed(commandList.Context, pt_heap_set_buffer(commandList.Context, heapNext + 1, di, hg.indices.size(), hg.indexStride));
                GeometryOnDevice od{ heapNext, heapNext + 1, ~0u, dv, nullptr, nullptr, hg.vertexCount }; heapNext += 2;
                if (!hg.skeletal.empty()) {                                  // Mesh::SkeletalVertices + Mesh::MotionVectors (GLTFHelpers.ixx:342-345)
                    od.skeletal = upload(hg.skeletal); od.motion = upload(std::vector<uint8_t>((size_t)hg.vertexCount * 8, 0)); od.heapMotion = motionNext++;
                    ThrowIfFailed(commandList.Context, pt_heap_set_buffer(commandList.Context, od.heapMotion, od.motion, (uint64_t)hg.vertexCount * 8, 8));
                    skeletal = true;
                }
                onDevice[ni].push_back(od);
                // Scene.ixx:320-324: FLAG_OPAQUE unless the material is alpha-tested / blended
                geoms.push_back(RaytracingHelpers::CreateGeometryDesc({ dv, hg.vertexCount, sizeof(Vertex) }, { di, hg.indexCount, hg.indexStride },
                                                                      hg.material.AlphaMode == 0 ? PT_GEOMETRY_FLAG_OPAQUE : 0u));
            }
            // Scene.ixx:329: skeletal mesh nodes are built PREFER_FAST_BUILD | ALLOW_UPDATE, static ones PREFER_FAST_TRACE
            blas[ni] = RaytracingHelpers::BuildBottomLevelAccelerationStructure(commandList, geoms, skeletal ? (PT_BUILD_FLAG_PREFER_FAST_BUILD | PT_BUILD_FLAG_ALLOW_UPDATE) : PT_BUILD_FLAG_PREFER_FAST_TRACE);
        }
        // ---- ObjectData / InstanceData (App::UpdateScene, Source/App.cpp:1028-1074): one object record per (instance, geometry), InstanceID = the
        // instance's first object (Scene.ixx:371)
        std::vector<PtObjectData> objectData; std::vector<PtInstanceData> instanceData(scene.objects.size());
        std::vector<PtInstanceDesc> instanceDescs(scene.objects.size());
        for (size_t i = 0; i < scene.objects.size(); i++) {
            const HostObject& ho = scene.objects[i];
            const uint32_t first = (uint32_t)objectData.size();
            for (size_t g = 0; g < scene.nodes[ho.node].meshes.size(); g++) {
                const HostGeometry& hg = scene.nodes[ho.node].meshes[g];
                PtObjectData od; memset(&od, 0, sizeof od);
                od.VertexDesc.Stride = sizeof(Vertex);
                od.VertexDesc.AttributeOffsets.Normal = hg.hasNormals ? 12u : ~0u; od.VertexDesc.AttributeOffsets.Tangent = hg.hasTangents ? 18u : ~0u;
                od.VertexDesc.AttributeOffsets.TextureCoordinates[0] = hg.hasUV[0] ? 24u : ~0u; od.VertexDesc.AttributeOffsets.TextureCoordinates[1] = hg.hasUV[1] ? 28u : ~0u;
                od.MeshDescriptors.Vertices = onDevice[ho.node][g].heapVertices; od.MeshDescriptors.Indices = onDevice[ho.node][g].heapIndices; od.MeshDescriptors.MotionVectors = onDevice[ho.node][g].heapMotion;
                od.Material = hg.material;
                for (int k = 0; k < 7; k++) {
                    od.TextureMapInfoArray[k].Descriptor = hg.textures[k] ? textureDescriptor[hg.textures[k].get()] : ~0u;
                    od.TextureMapInfoArray[k].TextureCoordinateIndex = hg.texCoord[k];
                }
                objectData.push_back(od);
            }
            PtInstanceData& id = instanceData[i]; memset(&id, 0, sizeof id);
            id.FirstGeometryIndex = first;
            memcpy(id.ObjectToWorld, ho.transform, 48); memcpy(id.PreviousObjectToWorld, ho.transform, 48);
            PtInstanceDesc& d = instanceDescs[i]; memset(&d, 0, sizeof d);
            memcpy(d.Transform, ho.transform, 48); d.InstanceID = first; d.InstanceMask = ho.visible ? ~0u : 0u; d.AccelerationStructure = blas[ho.node];
        }
        const uint32_t n = (uint32_t)objectData.size(), nInstances = (uint32_t)scene.objects.size();
        RaytracingHelpers::TopLevelAccelerationStructure tlas;
        RaytracingHelpers::BuildTopLevelAccelerationStructure(commandList, PT_BUILD_FLAG_PREFER_FAST_TRACE, instanceDescs, false, tlas);
        PtObjectData* dObjects = upload(objectData); PtInstanceData* dInstances = upload(instanceData);

        // ---- camera (scenes.py:make_camera: hfov 90, near 0.01, far inf) and scene data
        PtCamera cam = make_camera(scene, (double)outW / (double)outH);
        PtSceneData sd{}; sd.IsStatic = scene.animations.empty() ? 1 : 0; sd.EnvironmentLightTextureDescriptor = ~0u;
        memcpy(sd.EnvironmentLightColor, scene.envColor, 16); memcpy(sd.EnvironmentLightTransform, scene.envTransform, 48);

        // ---- textures (Source/App.cpp:438-455 formats)
        const size_t px_ = (size_t)W * std::max(localRows, 1u), fullPx = (size_t)W * H;     // a rank's textures hold its own rows
        const size_t outPx = (size_t)outW * outH;                  // the frame the post chain sees: the upscaler's output, else the render size
        PtTextures tx{}; float* radianceF32 = nullptr;
        auto alloc = [&](size_t bytes) { void* p = nullptr; HIP_OK(hipMalloc(&p, bytes)); HIP_OK(hipMemset(p, 0, bytes)); return p; };
        tx.Position = alloc(px_ * 16); tx.FlatNormal = alloc(px_ * 4); tx.GeometricNormal = alloc(px_ * 4); tx.LinearDepth = alloc(px_ * 4);
        tx.NormalizedDepth = alloc(px_ * 4); tx.MotionVector = alloc(px_ * 8); tx.BaseColorMetalness = alloc(px_ * 4); tx.NormalRoughness = alloc(px_ * 8);
        tx.IOR = alloc(px_ * 2); tx.Transmission = alloc(px_); tx.Radiance = alloc(px_ * 8);
        tx.RadianceF32 = radianceF32 = (float*)alloc(px_ * 16);
        uint32_t nrdDenoiser = PT_DENOISER_NONE;
        if (nrd == "relax") nrdDenoiser = PT_DENOISER_NRD_RELAX;
        else if (nrd == "reblur") nrdDenoiser = PT_DENOISER_NRD_REBLUR;
        else if (!nrd.empty()) throw std::invalid_argument("--nrd: relax or reblur");
        if (di || nrdDenoiser) { tx.Diffuse = alloc(px_ * 8); tx.Specular = alloc(px_ * 8); }   // Raytracing::Textures Diffuse / Specular (App.cpp:475-482)
        // the Denoiser value of the frame: the NRD one, or DLSS-RR under --reconstruct (the guides the same, Radiance the noisy sum)
        const uint32_t frameDenoiser = reconstructing ? (uint32_t)PT_DENOISER_DLSS_RAY_RECONSTRUCTION : nrdDenoiser;
        if (frameDenoiser) { tx.DiffuseAlbedo = alloc(px_ * 8); tx.SpecularAlbedo = alloc(px_ * 8); }   // App.cpp:1223: the albedos exist for the denoiser
        void* fullRadiance = sharded && rank == 0 ? alloc(fullPx * 8) : nullptr;      // the assembled frame (R16G16B16A16_FLOAT), root only
        // ---- App::PostProcessGraphics (Denoiser::None): on the whole frame, rank 0 of a sharded run after the gather
        PostProcessing postProcessing(commandList);
        const bool runPost = post && rank == 0;
        if (post) {
            if (hdr && !pngPath.empty()) throw std::invalid_argument("--png writes an SDR image: drop --hdr");
            PostProcessing::Settings ps; ps.RenderSize[0] = outW; ps.RenderSize[1] = outH;
            ps.Bloom.IsEnabled = bloom; ps.Bloom.Strength = bloomStrength; ps.IsHDREnabled = hdr;
            using Op = PostProcessing::ToneMapOperator; using Rot = PostProcessing::ColorRotation;
            if (toneMap == "saturate") ps.ToneMapping.NonHDR.Operator = Op::Saturate;
            else if (toneMap == "reinhard") ps.ToneMapping.NonHDR.Operator = Op::Reinhard;
            else if (toneMap == "aces") ps.ToneMapping.NonHDR.Operator = Op::ACESFilmic;
            else throw std::invalid_argument("--tone-map: saturate, reinhard or aces");
            ps.ToneMapping.NonHDR.Exposure = exposure; ps.ToneMapping.HDR.PaperWhiteNits = paperWhite;
            if (colorRotation == "hdtv_to_uhdtv") ps.ToneMapping.HDR.ColorPrimaryRotation = Rot::HDTVtoUHDTV;
            else if (colorRotation == "dci_p3_d65_to_uhdtv") ps.ToneMapping.HDR.ColorPrimaryRotation = Rot::DCI_P3_D65toUHDTV;
            else if (colorRotation == "hdtv_to_dci_p3_d65") ps.ToneMapping.HDR.ColorPrimaryRotation = Rot::HDTVtoDCI_P3_D65;
            else throw std::invalid_argument("--color-rotation: hdtv_to_uhdtv, dci_p3_d65_to_uhdtv or hdtv_to_dci_p3_d65");
            postProcessing.SetConstants(ps);
            if (runPost) {
                postProcessing.Textures.Radiance = sharded ? fullRadiance : tx.Radiance;
                postProcessing.Textures.Color = alloc(outPx * 8);
                postProcessing.Textures.BackBuffer = alloc(outPx * 4);
                postProcessing.Textures.Display8 = alloc(outPx * 4);
            }
        }
        float* fullRadianceF32 = sharded && rank == 0 && !out.empty() ? (float*)alloc(fullPx * 16) : nullptr;

        // ---- App::RenderScene
        GBufferGeneration gbuffer(commandList);
        gbuffer.GPUBuffers = { &sd, &cam, dInstances, dObjects, nInstances, n };
        gbuffer.Textures = tx;
        Raytracing raytracing(commandList);
        raytracing.GPUBuffers = { &sd, &cam, dObjects, n };
        raytracing.Textures = tx;
        DirectLighting directLighting(commandList);
        directLighting.GPUBuffers = { &sd, &cam, dObjects, n };
        directLighting.Textures = tx;
        if (restir && (!di || sharded)) throw std::invalid_argument("--restir needs --di and one unsharded process");
        if (restirVisibility && !restir) throw std::invalid_argument("--restir-visibility needs --restir");
        if (restirRaytraced && !restirVisibility) throw std::invalid_argument("--restir-raytraced needs --restir-visibility");
        if (restirPairwise && !restir) throw std::invalid_argument("--restir-pairwise needs --restir");
        if (restirPairwise && restirRaytraced) throw std::invalid_argument("--restir-pairwise and --restir-raytraced are two bias corrections: give one");
        if (useSharc && sharded) throw std::invalid_argument("--sharc needs one unsharded process");
        if (useSharc && nrdDenoiser) throw std::invalid_argument("--nrd: the radiance-cache query does not serve the NRD packing, drop --sharc");
        NRDComposition nrdComposition(commandList);
        if (denoise && (!nrdDenoiser || sharded)) throw std::invalid_argument("--denoise needs --nrd relax and one unsharded process");
        Denoiser denoiser(commandList);
        if (denoise) {                                              // refuses ReBLUR's packing
            Denoiser::Settings s; s.RenderSize[0] = W; s.RenderSize[1] = H; s.Denoiser = nrdDenoiser;
            s.MaxAccumulatedFrames = denoiseFramesMax; s.AtrousIterations = denoiseIterations;
            denoiser.SetConstants(s);
        } else if (nrdDenoiser) fprintf(stderr, "pt_demo: --nrd %s: the denoiser between the pack and the compose is the identity\n", nrd.c_str());
        Upscaler upscaler(commandList);
        if (upscaling) {                                            // App.cpp:1532-1541: the super-resolution step, ahead of Bloom / ToneMap
            Upscaler::Settings s; s.RenderSize[0] = W; s.RenderSize[1] = H; s.OutputSize[0] = outW; s.OutputSize[1] = outH;
            upscaler.SetConstants(s);
            upscaler.Textures = { tx.Radiance, tx.LinearDepth, tx.MotionVector, alloc(outPx * 8) };
            if (runPost) postProcessing.Textures.Radiance = upscaler.Textures.Color;
        }
        Reconstruction reconstruction(commandList);
        if (reconstructing) {                                       // App.cpp:1513-1523: ProcessDLSSRayReconstruction's place, ahead of Bloom / ToneMap
            Reconstruction::Settings s; s.RenderSize[0] = W; s.RenderSize[1] = H; s.OutputSize[0] = outW; s.OutputSize[1] = outH;
            if (reconstructIterations != -1) s.AtrousIterations = (uint32_t)reconstructIterations;
            reconstruction.SetConstants(s);
            reconstruction.Textures = { tx.Radiance, tx.DiffuseAlbedo, tx.SpecularAlbedo, tx.NormalRoughness, tx.Position, tx.LinearDepth, tx.MotionVector,
                                        alloc(outPx * 8) };
            if (runPost) postProcessing.Textures.Radiance = reconstruction.Textures.Color;
        }
        Sharpening sharpening(commandList);
        const bool runSharpen = sharpen && rank == 0;
        if (runSharpen) {                                           // App.cpp:1544-1548: ProcessNIS's place, between the upscaler and Bloom
            Sharpening::Settings s; s.Size[0] = outW; s.Size[1] = outH; s.Sharpness = sharpness;
            sharpening.SetConstants(s);
            sharpening.Textures = { upscaling ? upscaler.Textures.Color : reconstructing ? reconstruction.Textures.Color : sharded ? fullRadiance : tx.Radiance,
                                    alloc(outPx * 8) };
            if (runPost) postProcessing.Textures.Radiance = sharpening.Textures.Sharpened;
        }
        FrameGeneration generation(commandList);
        bool generated = false;                                     // the last frame's Generated is an interpolated frame
        if (frameGeneration) {                                      // App.cpp:1564-1566: behind ToneMap, where the reference tags DLSS-G's inputs
            FrameGeneration::Settings s; s.RenderSize[0] = W; s.RenderSize[1] = H; s.OutputSize[0] = outW; s.OutputSize[1] = outH; s.Phase = fgPhase;
            generation.SetConstants(s);
            generation.Textures = { postProcessing.Textures.Color, tx.LinearDepth, tx.MotionVector, alloc(outPx * 8), alloc(outPx * 4) };
        }
        SHARC sharc(commandList);
        Raytracing::SHARCSettings sharcSettings; sharcSettings.DownscaleFactor = sharcDownscale;
        if (useSharc) { sharc.Constants.SceneScale = sceneScale; sharc.Configure(); }
        if (lightSampling != "cdf") {
            using Mode = DirectLighting::ReSTIRDILocalLightSamplingMode;
            DirectLighting::LightSampling l;
            if (lightSampling == "uniform") l.InitialSampling.LocalLight.Mode = Mode::Uniform;
            else if (lightSampling == "power_ris") l.InitialSampling.LocalLight.Mode = Mode::Power_RIS;
            else if (lightSampling == "regir") l.InitialSampling.LocalLight.Mode = Mode::ReGIR_RIS;
            else throw std::invalid_argument("--light-sampling: cdf, uniform, power_ris or regir");
            if (!di) throw std::invalid_argument("--light-sampling needs --di");
            if (regirLayout == "onion") l.ReGIR.Layout = DirectLighting::ReGIRLayout::Onion;
            else if (regirLayout != "grid") throw std::invalid_argument("--regir-layout: grid or onion");
            if (regirLayout != "grid" && lightSampling != "regir") throw std::invalid_argument("--regir-layout needs --light-sampling regir");
            directLighting.SetLightSampling(l);
        } else if (regirLayout != "grid") throw std::invalid_argument("--regir-layout needs --light-sampling regir");
        if (diPdfMipmap) {                                                        // the LocalLightPDF texture and its chain (App::PrepareReSTIRDI)
            if (!di) throw std::invalid_argument("--di-pdf-mipmap needs --di");
            directLighting.SetPdfMipmap(true);
        }
        if (diBrdfSamples || diBrdfCutoff != 0.0f) {                              // BRDF candidates in initial sampling (MyAppData BRDFSamples)
            if (!di) throw std::invalid_argument("--di-brdf-samples needs --di");
            if (!diBrdfSamples) throw std::invalid_argument("--di-brdf-cutoff needs --di-brdf-samples");
            DirectLighting::BrdfSampling b; b.Samples = diBrdfSamples; b.Cutoff = diBrdfCutoff;
            directLighting.SetBrdfSampling(b);
        }
        PtDIPreviousTextures& prev = directLighting.PreviousTextures;
        if (restir) {
            prev.PreviousGeometricNormal = alloc(px_ * 4); prev.PreviousLinearDepth = alloc(px_ * 4); prev.PreviousBaseColorMetalness = alloc(px_ * 4);
            prev.PreviousNormalRoughness = alloc(px_ * 8); prev.PreviousIOR = alloc(px_ * 2); prev.PreviousTransmission = alloc(px_);
            DirectLighting::ReSTIRDI r;
            r.TemporalResampling.IsEnabled = true; r.SpatialResampling.IsEnabled = true;
            if (restirPairwise) r.TemporalResampling.BiasCorrectionMode = r.SpatialResampling.BiasCorrectionMode = DirectLighting::ReSTIRDIBiasCorrectionMode::Pairwise;
            directLighting.SetResampling(r);
            if (restirVisibility) {
                DirectLighting::Visibility v;
                v.TemporalRaytraced = v.SpatialRaytraced = restirRaytraced;
                directLighting.SetVisibility(v);
            }
        }
        // ---- animation: one rig per animation file, one collection per animated render object; a frame's update is Scene::Tick / Refresh /
        // SkinSkeletalMeshes / CreateAccelerationStructures (Scene.ixx:174-188), all of it enqueued
        std::map<const ingest::Rig*, std::shared_ptr<AnimationRig>> rigs;
        std::vector<std::unique_ptr<AnimationCollection>> collections; std::vector<AnimationCollection*> collectionList;
        std::vector<uint8_t> fromDevice(nInstances, 0);
        SkeletalMeshSkinning skinning(commandList);
        if (animate) {
            ThrowIfFailed(commandList.Context, pt_set_instance_data(commandList.Context, dInstances, nInstances));
            for (const ingest::AnimatedObject& ao : scene.animations) {
                const ingest::Rig& r = *ao.Animation;
                if (!rigs.count(&r)) rigs[&r] = std::make_shared<AnimationRig>(commandList, AnimationRig::Desc{ r.Parents, r.Rest, r.Durations, r.Channels, r.KeyTimes, r.KeyValues });
                std::vector<uint32_t> skinNodes, jointCounts, jointNodes; std::vector<float> inverseBinds;
                for (const auto& sk : ao.Skins) {
                    skinNodes.push_back(sk.MeshNode); jointCounts.push_back((uint32_t)sk.JointNodes.size());
                    jointNodes.insert(jointNodes.end(), sk.JointNodes.begin(), sk.JointNodes.end()); inverseBinds.insert(inverseBinds.end(), sk.InverseBinds.begin(), sk.InverseBinds.end());
                }
                collections.push_back(std::make_unique<AnimationCollection>(commandList, rigs[&r], AnimationCollection::Bindings{ std::span<const float>(ao.Transform, 16), ao.BindingNodes, ao.BindingInstances,
                                                                                                                               ao.BindingGlobals, skinNodes, jointCounts, jointNodes, inverseBinds }));
                collectionList.push_back(collections.back().get());
                for (uint32_t i : ao.BindingInstances) fromDevice[i] = 1;
                AnimationCollection& c = *collections.back();
                c[c.GetSelectedIndex()].SetTime(animTime);
            }
        }
        auto animateFrame = [&] {
            if (collectionList.empty()) return;
            AnimationCollection::Evaluate(commandList, collectionList, dInstances);
            for (size_t a = 0; a < scene.animations.size(); a++)
                for (size_t k = 0; k < scene.animations[a].Skins.size(); k++) {
                    const uint32_t ni = scene.animations[a].Skins[k].SceneNode;
                    const GPUBuffer transforms = collections[a]->GetSkeletalTransforms((uint32_t)k);
                    for (const GeometryOnDevice& g : onDevice[ni]) {
                        if (!g.skeletal) continue;
                        const GPUBuffer sv{ g.skeletal, g.vertexCount, 48 }, vb{ g.vertices, g.vertexCount, sizeof(Vertex) }, mv{ g.motion, g.vertexCount, 8 };
                        skinning.GPUBuffers = { &sv, &transforms, &vb, &mv };
                        skinning.Process(commandList);
                    }
                    RaytracingHelpers::UpdateBottomLevelAccelerationStructure(commandList, blas[ni], nodeGeoms[ni], PT_BUILD_FLAG_PREFER_FAST_BUILD | PT_BUILD_FLAG_ALLOW_UPDATE);
                }
            RaytracingHelpers::BuildTopLevelAccelerationStructure(commandList, PT_BUILD_FLAG_PREFER_FAST_TRACE, instanceDescs, dInstances, fromDevice, tlas);
        };
        bool firstFrame = true;
        PtCounters counters{};
        double ms = 0;
        uint32_t poseIndex = 0;                                     // --camera-step: which frame of the camera's path renderFrame renders
        auto renderFrame = [&](uint32_t frameIndex) {
            float jitter[2] = { 0.0f, 0.0f };
            if (cameraMoves) {                                      // sideways along world x; the first pose is its own predecessor
                const double x = cameraStart + cameraStep * poseIndex;
                const double now[3] = { scene.cameraPosition[0] + x, scene.cameraPosition[1], scene.cameraPosition[2] };
                const double before[3] = { scene.cameraPosition[0] + (poseIndex ? x - cameraStep : x), scene.cameraPosition[1], scene.cameraPosition[2] };
                cam = make_moved_camera(scene, (double)outW / (double)outH, now, before);
            }
            if (resizing) {                                         // App.cpp:556: the frame's Halton jitter, in the camera every pass reads
                const uint32_t render[2] = { W, H }, output[2] = { outW, outH };
                Upscaler::Jitter(frameIndex, render, output, jitter);
                cam.Jitter[0] = jitter[0]; cam.Jitter[1] = jitter[1];
            }
            if (restir && !firstFrame) {                            // App.cpp:629-634: this frame's G-buffer goes where last frame's was
                std::swap(tx.GeometricNormal, prev.PreviousGeometricNormal); std::swap(tx.LinearDepth, prev.PreviousLinearDepth);
                std::swap(tx.BaseColorMetalness, prev.PreviousBaseColorMetalness); std::swap(tx.NormalRoughness, prev.PreviousNormalRoughness);
                std::swap(tx.IOR, prev.PreviousIOR); std::swap(tx.Transmission, prev.PreviousTransmission);
                gbuffer.Textures = tx; raytracing.Textures = tx; directLighting.Textures = tx;
            }
            firstFrame = false;
            gbuffer.Render(commandList, tlas, { { W, H }, frameDenoiser ? ~0u : ~0u & ~(uint32_t)GBufferGeneration::Flags::Albedo });     // App.cpp:1223-1224
            if (di) {                                               // App.cpp:1234-1308: RTXDI between the G-buffer and the path tracer
                DirectLighting::Settings ds; ds.RenderSize[0] = W; ds.RenderSize[1] = H; ds.FrameIndex = frameIndex;
                ds.LocalLightSamples = diSamples; ds.IsLastRenderPass = bounces == 0; ds.Denoiser = frameDenoiser;
                directLighting.SetConstants(ds);
                directLighting.Render(commandList, tlas);
            }
            Raytracing::GraphicsSettings gs; gs.RenderSize[0] = W; gs.RenderSize[1] = H;
            gs.FrameIndex = frameIndex; gs.Bounces = bounces; gs.SamplesPerPixel = spp; gs.IsRussianRouletteEnabled = true;
            gs.IsDIEnabled = di; gs.Denoiser = frameDenoiser;
            raytracing.SetConstants(gs);
            if (useSharc) raytracing.Render(commandList, tlas, sharc, sharcSettings);
            else raytracing.Render(commandList, tlas);
            if (nrdDenoiser) {                                      // App::ProcessNRD (App.cpp:1595-1688): pack, the denoiser (the identity), compose
                NRDComposition::Constants nc; nc.RenderSize[0] = W; nc.RenderSize[1] = std::max(localRows, 1u); nc.Denoiser = nrdDenoiser;
                nrdComposition.Textures = { tx.LinearDepth, tx.DiffuseAlbedo, tx.SpecularAlbedo, tx.NormalRoughness, tx.Diffuse, tx.Specular,
                                            tx.Diffuse, tx.Specular, tx.Radiance };
                nc.IsPack = true; nrdComposition.Process(commandList, nc);
                if (denoise) {                                      // in place: the Denoised pair is the Noisy pair
                    denoiser.Textures = { tx.Position, tx.LinearDepth, tx.NormalRoughness, tx.MotionVector, tx.Diffuse, tx.Specular, tx.Diffuse, tx.Specular };
                    denoiser.Process(commandList);
                }
                nc.IsPack = false; nrdComposition.Process(commandList, nc);
            }
            if (sharded) sharding.GatherBands(commandList, tx.Radiance, fullRadiance, W, H, 8);
            if (upscaling) upscaler.Process(commandList, jitter);
            if (reconstructing) {                                   // the restir swap may have moved the G-buffer textures
                reconstruction.Textures.NormalRoughness = tx.NormalRoughness; reconstruction.Textures.LinearDepth = tx.LinearDepth;
                reconstruction.Process(commandList, jitter);
            }
            if (runSharpen) sharpening.Process(commandList);
            if (runPost) postProcessing.Render(commandList);
            if (frameGeneration) {                                  // the restir swap may have moved LinearDepth
                generation.Textures.LinearDepth = tx.LinearDepth;
                generated = generation.Process(commandList, jitter);
            }
        };
        animateFrame();
        renderFrame(12345);                                         // warm-up
        commandList.End();
        if (denoise) denoiser.ResetHistory();                       // the warm-up frame is not part of the sequence
        if (upscaling) upscaler.ResetHistory();
        if (reconstructing) reconstruction.ResetHistory();
        if (frameGeneration) generation.ResetHistory();
        // timed run: frames 1..N back to back
        ThrowIfFailed(commandList.Context, pt_reset_counters(commandList.Context));
        const auto t0 = std::chrono::steady_clock::now();
        for (uint32_t f = 0; f < frames; f++) {                    // the last frame has FrameIndex 0 (dumped below)
            if (f) for (AnimationCollection* c : collectionList) (*c)[c->GetSelectedIndex()].Tick(animStep);
            animateFrame();
            poseIndex = f;
            renderFrame(denoise || resizing ? f : frames - 1 - f);  // a denoised or upscaled run is a temporal sequence: FrameIndex counts up
        }
        commandList.End();
        ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        ThrowIfFailed(commandList.Context, pt_get_counters(commandList.Context, &counters));
        const double rays = (double)(counters.PrimaryRays + counters.SecondaryRays);
        if (di) {                                                   // the direct-lighting pass's emissive triangles, on stderr
            uint32_t lights = 0;
            ThrowIfFailed(commandList.Context, pt_di_light_count(commandList.Context, &lights));
            fprintf(stderr, "pt_demo: direct lighting over %u emissive triangles, %u candidates per pixel\n", lights, diSamples);
        }
        const char* pdfField = diPdfMipmap ? ", \"di_pdf_mipmap\": true" : "";
        if (useSharc)        // rays count the update pass's too
            printf("{\"host\": \"c++\", \"sharc\": true, \"width\": %u, \"height\": %u, \"spp\": %u, \"bounces\": %u, \"frames\": %u, \"sharc_entries\": %u, \"secondary_rays\": %.0f, \"rays\": %.0f, \"ms_per_frame\": %.4f%s}\n",
                   W, H, spp, bounces, frames, sharc.LiveEntries(), (double)counters.SecondaryRays, rays, ms / frames, pdfField);
        else if (!sharded)
            printf("{\"host\": \"c++\", \"width\": %u, \"height\": %u, \"spp\": %u, \"bounces\": %u, \"frames\": %u, \"rays\": %.0f, \"ms_per_frame\": %.4f, \"mrays_per_s\": %.1f%s}\n",
                   W, H, spp, bounces, frames, rays, ms / frames, rays / ms / 1e3, pdfField);
        else       // rays are this rank's; rank 0's time includes every peer's bands arriving
            printf("{\"host\": \"c++\", \"rank\": %u, \"world\": %u, \"local_rows\": %u, \"width\": %u, \"height\": %u, \"spp\": %u, \"bounces\": %u, \"frames\": %u, \"rays_this_rank\": %.0f, \"ms_per_frame\": %.4f%s}\n",
                   rank, world, localRows, W, H, spp, bounces, frames, rays, ms / frames, pdfField);
        if (sharded && fullRadianceF32) {                          // parity dump of a sharded run: the fp32 copy, assembled the same way
            sharding.GatherBands(commandList, radianceF32, fullRadianceF32, W, H, 16);
            commandList.End();
        } else if (sharded && !out.empty() && rank != 0) {
            sharding.GatherBands(commandList, radianceF32, nullptr, W, H, 16);
            commandList.End();
        }
        if (!out.empty() && rank == 0) {                            // last frame rendered has FrameIndex 0
            std::vector<float> host(fullPx * 4);
            HIP_OK(hipMemcpy(host.data(), fullRadianceF32 ? fullRadianceF32 : radianceF32, fullPx * 16, hipMemcpyDeviceToHost));
            FILE* fp = fopen(out.c_str(), "wb");
            if (!fp) { fprintf(stderr, "cannot open %s\n", out.c_str()); return 3; }
            fwrite(host.data(), 16, fullPx, fp); fclose(fp);
        }
        if (!radiancePath.empty() && rank == 0) {                   // the fp16 Radiance of the last frame, whole frame
            std::vector<uint16_t> host(fullPx * 4);
            HIP_OK(hipMemcpy(host.data(), sharded ? fullRadiance : tx.Radiance, fullPx * 8, hipMemcpyDeviceToHost));
            FILE* fp = fopen(radiancePath.c_str(), "wb");
            if (!fp || fwrite(host.data(), 8, fullPx, fp) != fullPx) { fprintf(stderr, "cannot write %s\n", radiancePath.c_str()); if (fp) fclose(fp); return 3; }
            fclose(fp);
        }
        if (upscaling && !upscaledPath.empty()) {                   // the upscaler's Color of the last frame
            std::vector<uint16_t> host(outPx * 4);
            HIP_OK(hipMemcpy(host.data(), upscaler.Textures.Color, outPx * 8, hipMemcpyDeviceToHost));
            FILE* fp = fopen(upscaledPath.c_str(), "wb");
            if (!fp || fwrite(host.data(), 8, outPx, fp) != outPx) { fprintf(stderr, "cannot write %s\n", upscaledPath.c_str()); if (fp) fclose(fp); return 3; }
            fclose(fp);
        }
        if (reconstructing && !reconstructedPath.empty()) {         // the reconstruction's Color of the last frame
            std::vector<uint16_t> host(outPx * 4);
            HIP_OK(hipMemcpy(host.data(), reconstruction.Textures.Color, outPx * 8, hipMemcpyDeviceToHost));
            FILE* fp = fopen(reconstructedPath.c_str(), "wb");
            if (!fp || fwrite(host.data(), 8, outPx, fp) != outPx) { fprintf(stderr, "cannot write %s\n", reconstructedPath.c_str()); if (fp) fclose(fp); return 3; }
            fclose(fp);
        }
        if (runSharpen && !sharpenedPath.empty()) {                 // the sharpener's output of the last frame
            std::vector<uint16_t> host(outPx * 4);
            HIP_OK(hipMemcpy(host.data(), sharpening.Textures.Sharpened, outPx * 8, hipMemcpyDeviceToHost));
            FILE* fp = fopen(sharpenedPath.c_str(), "wb");
            if (!fp || fwrite(host.data(), 8, outPx, fp) != outPx) { fprintf(stderr, "cannot write %s\n", sharpenedPath.c_str()); if (fp) fclose(fp); return 3; }
            fclose(fp);
        }
        if (frameGeneration && !generated) throw std::runtime_error("--frame-generation: the last frame generated nothing");
        if (frameGeneration && !generatedPath.empty()) {            // the frame between the last two rendered ones
            std::vector<uint16_t> host(outPx * 4);
            HIP_OK(hipMemcpy(host.data(), generation.Textures.Generated, outPx * 8, hipMemcpyDeviceToHost));
            FILE* fp = fopen(generatedPath.c_str(), "wb");
            if (!fp || fwrite(host.data(), 8, outPx, fp) != outPx) { fprintf(stderr, "cannot write %s\n", generatedPath.c_str()); if (fp) fclose(fp); return 3; }
            fclose(fp);
        }
        if (frameGeneration && !generatedPngPath.empty()) {
            std::vector<uint8_t> rgba(outPx * 4);
            HIP_OK(hipMemcpy(rgba.data(), generation.Textures.Generated8, outPx * 4, hipMemcpyDeviceToHost));
            if (!ptpng::write_rgb(generatedPngPath, rgba.data(), outW, outH)) { fprintf(stderr, "cannot write %s\n", generatedPngPath.c_str()); return 3; }
        }
        if (runPost && !displayPath.empty()) {                      // the presented back buffer of the last frame
            std::vector<uint32_t> words(outPx);
            HIP_OK(hipMemcpy(words.data(), postProcessing.Textures.BackBuffer, outPx * 4, hipMemcpyDeviceToHost));
            FILE* fp = fopen(displayPath.c_str(), "wb");
            if (!fp || fwrite(words.data(), 4, outPx, fp) != outPx) { fprintf(stderr, "cannot write %s\n", displayPath.c_str()); if (fp) fclose(fp); return 3; }
            fclose(fp);
        }
        if (runPost && !pngPath.empty()) {
            std::vector<uint8_t> rgba(outPx * 4);
            HIP_OK(hipMemcpy(rgba.data(), postProcessing.Textures.Display8, outPx * 4, hipMemcpyDeviceToHost));
            if (!ptpng::write_rgb(pngPath, rgba.data(), outW, outH)) { fprintf(stderr, "cannot write %s\n", pngPath.c_str()); return 3; }
        }
    } catch (const std::exception& e) {
        fprintf(stderr, "pt_demo: %s\n", e.what());
        return 1;
    }
    return 0;
}
