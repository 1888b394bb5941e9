"""Developer helper: time the NRD composition pass (pt_nrd_composition_process). Pack and compose for ReLAX and ReBLUR at 1920 x 1080 and
3840 x 2160, in both launch forms (two pixels per lane with 16-byte accesses: what the library launches for textures aligned to two texels;
one pixel per lane with 8-byte accesses: what it launches otherwise, reached here through views that start one texel into their
allocation), each launch between two HIP events, median of --n launches after a warm-up. Beside every case, in the same
process, a hipMemcpyAsync device-to-device copy sized so that it reads and writes as many bytes as the pass, timed the same way.
Bytes per pixel (every LinearDepth finite):
    pack ReLAX     36 read (LinearDepth 4, two albedos 16, NoisyDiffuse / NoisySpecular 16) + 16 written = 52
    pack ReBLUR    44 read (the same + NormalRoughness 8)                                    + 16 written = 60
    compose        44 read (LinearDepth 4, two albedos 16, the denoised pair 16, Radiance 8) +  8 written = 52   (either denoiser)
so the copy moves 26, 30 and 26 bytes per pixel (a copy of n bytes reads n and writes n). Then a C2 frame (Cornell box, 4 spp, 8 bounces,
Denoiser ReLAX, one frame in flight) with and without the two passes. One JSON line per case, also appended to --out.
usage: tools/nrd_time.py [--sizes 1920x1080,3840x2160] [--n 50] [--frames 10] [--no-c2] [--out profiles/nrd/nrd_time.jsonl]"""
import argparse, ctypes as C, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BYTES = {("pack", "relax"): (36, 16), ("pack", "reblur"): (44, 16), ("compose", "relax"): (44, 8), ("compose", "reblur"): (44, 8)}


def hip_runtime():
    """the HIP runtime this process already uses (torch's), for hipMemcpyAsync"""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return C.CDLL(line.split()[-1])
    raise SystemExit("no HIP runtime is loaded")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1920x1080,3840x2160"); ap.add_argument("--n", type=int, default=50)
    ap.add_argument("--frames", type=int, default=10); ap.add_argument("--no-c2", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nrd", "nrd_time.jsonl"))
    a = ap.parse_args()
    if a.n < 20:
        raise SystemExit("--n: the median is taken over at least 20 launches")
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import __graft_entry__ as ge
    ge.load_package()
    import dxpbrt_amd.layouts as L, dxpbrt_amd.ptamd as P, dxpbrt_amd.scenes as S
    if not torch.cuda.is_available():
        raise SystemExit("nrd_time.py measures on the GPU: none is visible")
    ctx = P.DeviceContext(0)
    dev = torch.device("cuda", 0)
    hip = hip_runtime()
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    log = open(a.out, "a")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True); log.write(line + "\n"); log.flush()

    def median_us(fn, n):
        """each call between two events of its own on the stream the library and the copy use (the null stream)"""
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
        for b, e in ev:
            b.record(); fn(); e.record()
        torch.cuda.synchronize()
        return statistics.median(b.elapsed_time(e) for b, e in ev) * 1e3

    op = P.NRDComposition(ctx)
    rng = np.random.default_rng(1)
    for size in a.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        px = W * H

        def device(host):
            """(a tensor aligned to its allocation, the same values in a view that starts one texel in: aligned to one texel, not to two)"""
            t = torch.from_numpy(host).to(dev)
            lead = 4 if host.ndim == 3 else 1
            odd = torch.zeros(lead + t.numel(), dtype=t.dtype, device=dev)[lead:].view(t.shape)
            odd.copy_(t)
            return t, odd

        def half4(lo, hi):
            return device(rng.uniform(lo, hi, (H, W, 4)).astype(np.float16).view(np.int16))
        both = {"LinearDepth": device(rng.uniform(0.5, 20.0, (H, W)).astype(np.float32)),
                "DiffuseAlbedo": half4(0.01, 1.0), "SpecularAlbedo": half4(0.01, 1.0),
                "NormalRoughness": device(rng.integers(0, 32768, (H, W, 4)).astype(np.int16)),
                "NoisyDiffuse": half4(0.0, 4.0), "NoisySpecular": half4(0.0, 4.0), "Radiance": half4(0.0, 1.0),
                "DenoisedDiffuse": half4(0.0, 4.0), "DenoisedSpecular": half4(0.0, 4.0)}
        forms = {"two_pixels": {k: v[0] for k, v in both.items()}, "one_pixel": {k: v[1] for k, v in both.items()}}
        fresh = {k: both[k][0].clone() for k in ("NoisyDiffuse", "NoisySpecular", "Radiance")}
        src = torch.empty(30 * px, dtype=torch.uint8, device=dev); dst = torch.empty_like(src)
        for name, den in (("relax", L.DENOISER_NRD_RELAX), ("reblur", L.DENOISER_NRD_REBLUR)):
            for what in ("pack", "compose"):
                rd, wr = BYTES[(what, name)]
                nbytes = (rd + wr) * px
                k = L.nrd_composition_constants(W, H, den, what == "pack")
                us = {}
                for form, tex in forms.items():
                    for t in fresh:
                        tex[t].copy_(fresh[t])
                    us[form] = median_us(lambda: op.Process(tex, k), a.n)
                copy_us = median_us(lambda: hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), nbytes // 2, 3, None), a.n)
                emit({"size": [W, H], "pass": what, "denoiser": name, "read_B_per_px": rd, "written_B_per_px": wr, "MB_moved": round(nbytes / 1e6, 2),
                      "us_two_pixels_per_lane": round(us["two_pixels"], 2), "us_one_pixel_per_lane": round(us["one_pixel"], 2), "launches_timed": a.n,
                      "copy_bytes": nbytes // 2, "us_same_bytes_copy": round(copy_us, 2), "ratio_to_copy": round(us["two_pixels"] / copy_us, 3),
                      "TB_per_s": round(nbytes / (us["two_pixels"] * 1e-6) / 1e12, 3)})
    if not a.no_c2:
        W, H = 1920, 1080
        ctx.set_frames_in_flight(1)
        g = P.Scene(ctx, S.cornell_box(aspect=W / H, variant="ggx"))
        r = P.Renderer(ctx, g, W, H, with_denoiser_outputs=True)
        gs = S.graphics_settings(W, H, spp=4, bounces=8)
        gs["Denoiser"] = L.DENOISER_NRD_RELAX

        def frame_ms(**kw):
            """one frame at a time: the host waits for each"""
            ms = []
            for _ in range(a.frames):
                b, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                b.record(); r.render(gs, **kw); e.record(); torch.cuda.synchronize()
                ms.append(b.elapsed_time(e))
            return statistics.median(ms)
        r.render(gs, nrd=L.DENOISER_NRD_RELAX); r.render(gs); ctx.sync()
        off = frame_ms(); on = frame_ms(nrd=L.DENOISER_NRD_RELAX); off2 = frame_ms()
        emit({"workload": "c2", "denoiser": "relax", "size": [W, H], "frame_ms_without_passes": round(min(off, off2), 4),
              "frame_ms_with_passes": round(on, 4), "passes_share": round((on - min(off, off2)) / on, 4)})
        g.close()
    ctx.close()


if __name__ == "__main__":
    main()
