"""Developer helper: time the temporal upscaler (pt_upscaler_process) and what a frame gains from rendering below the output size.

1. The pass alone at 960x540 -> 1920x1080, 1280x720 -> 1920x1080 and 1920x1080 -> 3840x2160, one launch per call, each call between two
   HIP events, median of --n calls after a warm-up, on a history that is 8 frames long; --runs runs per form, the direct form
   (PT_UPSCALER_FORM_DIRECT) and the staged form (PT_UPSCALER_FORM_STAGED) alternating. A form is the faster one when its slowest run is
   below the other's fastest. Beside it, in the same process, a hipMemcpyAsync device-to-device copy sized so that
   it reads and writes as many bytes as the pass must (a copy of n bytes reads n and writes n): per render pixel 20 read (Radiance 8,
   LinearDepth 4, MotionVector 8: each texel once, whatever the taps share), per output pixel 20 of the last history read, 20 of this
   frame's written and the 8 of Color.
2. A C2 frame (Cornell box, 4 spp, 8 bounces, Denoiser None, one frame in flight) with the post chain: rendered at 1920 x 1080, and
   rendered at 960 x 540 and at 1280 x 720 with the upscaler in front of the post chain at 1920 x 1080.
One JSON line per case, also appended to --out.
usage: tools/upscale_time.py [--n 30] [--runs 3] [--frames 10] [--no-c2] [--out profiles/upscale/upscale_time.jsonl]"""
import argparse, ctypes as C, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEBUG_DIRECT, DEBUG_STAGED = 0x2000, 0x4000
CASES = [((960, 540), (1920, 1080)), ((1280, 720), (1920, 1080)), ((1920, 1080), (3840, 2160))]


def hip_runtime():
    """the HIP runtime this process already uses (torch's), for hipMemcpyAsync"""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return C.CDLL(line.split()[-1])
    raise SystemExit("no HIP runtime is loaded")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=30); ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--frames", type=int, default=10); ap.add_argument("--no-c2", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "upscale", "upscale_time.jsonl"))
    a = ap.parse_args()
    if a.n < 20:
        raise SystemExit("--n: the median is taken over at least 20 calls")
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import __graft_entry__ as ge
    ge.load_package()
    import dxpbrt_amd.layouts as L, dxpbrt_amd.ptamd as P, dxpbrt_amd.scenes as S
    if not torch.cuda.is_available():
        raise SystemExit("upscale_time.py measures on the GPU: none is visible")
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
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
        for b, e in ev:
            b.record(); fn(); e.record()
        torch.cuda.synchronize()
        return statistics.median(b.elapsed_time(e) for b, e in ev) * 1e3

    op = P.Upscaler(ctx)
    rng = np.random.default_rng(1)
    for render, output in CASES:
        (Rw, Rh), (Ow, Oh) = render, output
        tex = {"Radiance": torch.from_numpy((1.0 + rng.uniform(-0.5, 0.5, (Rh, Rw, 4))).astype(np.float16).view(np.int16)).to(dev),
               "LinearDepth": torch.full((Rh, Rw), 5.0, dtype=torch.float32, device=dev),
               "MotionVector": torch.zeros((Rh, Rw, 4), dtype=torch.int16, device=dev),
               "Color": torch.empty((Oh, Ow, 4), dtype=torch.int16, device=dev)}
        nbytes = 20 * Rw * Rh + 48 * Ow * Oh
        src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev); dst = torch.empty_like(src)
        op.SetConstants(L.upscaler_settings(render, output, MaxAccumulatedFrames=8))
        jitters = [P.upscaler_jitter(f, render, output) for f in range(64)]
        state = {"f": 0}

        def call():
            op.Process(jitters[state["f"] % len(jitters)], tex)
            state["f"] += 1
        for _ in range(8):
            call()
        us = {"direct": [], "staged": []}
        for _ in range(a.runs):
            for form, flag in (("direct", DEBUG_DIRECT), ("staged", DEBUG_STAGED)):
                ctx.set_debug_flags(flag)
                us[form].append(round(median_us(call, a.n), 2))
        ctx.set_debug_flags(0)
        copy = median_us(lambda: hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), nbytes // 2, 3, None), a.n)
        faster = "direct" if max(us["direct"]) < min(us["staged"]) else "staged" if max(us["staged"]) < min(us["direct"]) else None
        best = min(us["direct"] + us["staged"])
        emit({"render": list(render), "output": list(output), "calls_timed": a.n, "bytes": nbytes, "us_direct": us["direct"], "us_staged": us["staged"],
              "faster_form": faster, "us_same_bytes_copy": round(copy, 2), "ratio_to_copy": round(best / copy, 3),
              "TB_per_s": round(nbytes / (best * 1e-6) / 1e12, 3), "history_B_per_output_px": 40})
    if not a.no_c2:
        out = (1920, 1080)
        ctx.set_frames_in_flight(1)
        g = P.Scene(ctx, S.cornell_box(aspect=out[0] / out[1], variant="ggx"))
        post = L.post_processing_settings(*out)

        def frame_ms(r, gs, up, render):
            """one frame at a time: the host waits for each"""
            ms = []
            for f in range(a.frames + 2):
                if up is not None:
                    g.desc.camera["Jitter"] = P.upscaler_jitter(f, render, out)
                b, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                b.record(); r.render(gs, post=post, upscale=up); e.record(); torch.cuda.synchronize()
                ms.append(b.elapsed_time(e))
            g.desc.camera["Jitter"] = (0.0, 0.0)
            return statistics.median(ms[2:])
        native = P.Renderer(ctx, g, *out)
        native_ms = [frame_ms(native, S.graphics_settings(*out, spp=4, bounces=8), None, out)]
        for render in ((960, 540), (1280, 720)):
            r = P.Renderer(ctx, g, *render)
            up = r.upscaler(*out)
            gs = S.graphics_settings(*render, spp=4, bounces=8)
            ms = frame_ms(r, gs, up, render)
            native_ms.append(frame_ms(native, S.graphics_settings(*out, spp=4, bounces=8), None, out))
            ref = min(native_ms)
            pixels = render[0] * render[1] / (out[0] * out[1])
            emit({"workload": "c2", "output": list(out), "render": list(render), "frame_ms_native": round(ref, 4), "frame_ms_upscaled": round(ms, 4),
                  "speedup": round(ref / ms, 3), "pixel_fraction": round(pixels, 4),
                  "saving_kept": round((ref - ms) / (ref * (1 - pixels)), 3)})
        g.close()
    ctx.close()


if __name__ == "__main__":
    main()
