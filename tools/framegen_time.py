"""Developer helper: time the frame interpolator (pt_frame_generation_process) and what a displayed frame costs beside a rendered one.

1. The whole call at 960x540 -> 1920x1080, 1920x1080 native and 1920x1080 -> 3840x2160 (the clear of the field, the scatter, the resolve
   and the history copy: five enqueued operations), each call between two HIP events, median of --n calls after a warm-up, on frames
   whose motion is a steady 1.5 render pixels. Beside it, in the same process, a hipMemcpyAsync device-to-device copy sized so that it
   reads and writes as many bytes as the call must (a copy of n bytes reads n and writes n): per output pixel two colour reads and one
   write (24 B), the history's copy of Color (8 read, 8 written), the class byte (1); per render pixel the field cleared, scattered and
   read (24 B), LinearDepth twice and MotionVector once (16 B), the history's copy of LinearDepth (4 read, 4 written).
   The three stages one by one are the rows of a kernel trace of this tool (k_fg_scatter, k_fg_resolve, the runtime's fill kernel):
   rocprofv3 --kernel-trace --stats -- python tools/framegen_time.py --no-c2
2. A C2 default-configuration chain (Cornell box, 4 spp, 8 bounces, rendered at 960 x 540, the upscaler and the post chain at 1920 x 1080,
   one frame in flight) without and with the pass: frame time, rendered frames per second, displayed frames per second (twice the
   rendered ones with the pass: one generated frame between every two). Then the reference's default configuration at the same sizes
   (tools/reconstruct_time.py's chain: DI with reservoir reuse, the radiance cache, Denoiser = DLSS-RR, the reconstruction, the post
   chain), without and with the pass.
One JSON line per case, also appended to --out.
usage: tools/framegen_time.py [--n 30] [--frames 10] [--no-c2] [--out profiles/framegen/framegen_time.jsonl]"""
import argparse, ctypes as C, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [((960, 540), (1920, 1080)), ((1920, 1080), (1920, 1080)), ((1920, 1080), (3840, 2160))]


def hip_runtime():
    """the HIP runtime this process already uses (torch's), for hipMemcpyAsync"""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return C.CDLL(line.split()[-1])
    raise SystemExit("no HIP runtime is loaded")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=30); ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--no-c2", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "framegen", "framegen_time.jsonl"))
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
        raise SystemExit("framegen_time.py measures on the GPU: none is visible")
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

    op = P.FrameGeneration(ctx)
    rng = np.random.default_rng(1)
    for render, output in CASES:
        (Rw, Rh), (Ow, Oh) = render, output
        mv = np.zeros((Rh, Rw, 4), np.float16); mv[..., 0] = 1.5
        tex = {"Color": torch.from_numpy((0.5 + rng.uniform(-0.4, 0.4, (Oh, Ow, 4))).astype(np.float16).view(np.int16)).to(dev),
               "LinearDepth": torch.full((Rh, Rw), 5.0, dtype=torch.float32, device=dev),
               "MotionVector": torch.from_numpy(mv.view(np.int16)).to(dev),
               "Generated": torch.empty((Oh, Ow, 4), dtype=torch.int16, device=dev), "Generated8": None}
        nbytes = (24 + 16 + 1) * Ow * Oh + (24 + 16 + 8) * Rw * Rh
        src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev); dst = torch.empty_like(src)
        op.SetConstants(L.frame_generation_settings(render, output))
        op.ResetHistory()
        jitters = [P.upscaler_jitter(f, render, output) for f in range(64)]
        state = {"f": 0}

        def call():
            op.Process(jitters[state["f"] % len(jitters)], tex)
            state["f"] += 1
        us = round(median_us(call, a.n), 2)
        classes = np.bincount(op.DownloadField()[1].ravel(), minlength=4).tolist()
        copy = median_us(lambda: hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), nbytes // 2, 3, None), a.n)
        emit({"render": list(render), "output": list(output), "calls_timed": a.n, "bytes": nbytes, "us_call": us,
              "us_same_bytes_copy": round(copy, 2), "ratio_to_copy": round(us / copy, 3), "TB_per_s": round(nbytes / (us * 1e-6) / 1e12, 3),
              "classes_both_current_previous_fallback": classes})
    if not a.no_c2:
        out, render = (1920, 1080), (960, 540)
        ctx.set_frames_in_flight(1)
        g = P.Scene(ctx, S.cornell_box(aspect=out[0] / out[1], variant="ggx"))
        post = L.post_processing_settings(*out)
        r = P.Renderer(ctx, g, *render)
        up = r.upscaler(*out)
        fg = r.frame_generation(*out)
        gs = S.graphics_settings(*render, spp=4, bounces=8)

        def frame_ms(generate):
            """one frame at a time: the host waits for each"""
            ms = []
            for f in range(a.frames + 2):
                g.desc.camera["Jitter"] = P.upscaler_jitter(f, render, out)
                b, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                b.record(); r.render(gs, post=post, upscale=up, generate=generate); e.record(); torch.cuda.synchronize()
                ms.append(b.elapsed_time(e))
            g.desc.camera["Jitter"] = (0.0, 0.0)
            return statistics.median(ms[2:])
        without = [frame_ms(None)]
        with_pass = frame_ms(fg)
        without.append(frame_ms(None))
        ref = min(without)
        emit({"workload": "c2", "render": list(render), "output": list(out), "frame_ms_without": round(ref, 4), "frame_ms_with": round(with_pass, 4),
              "pass_ms": round(with_pass - ref, 4), "rendered_fps_without": round(1e3 / ref, 1), "rendered_fps_with": round(1e3 / with_pass, 1),
              "displayed_fps_without": round(1e3 / ref, 1), "displayed_fps_with": round(2e3 / with_pass, 1)})
        # the reference's default configuration (tools/reconstruct_time.py's chain): DI with reservoir reuse, the radiance cache,
        # Denoiser = DLSS-RR, the reconstruction to the output size, the post chain; without and with the pass behind it
        r = P.Renderer(ctx, g, *render, with_denoiser_outputs=True, di_history=True)
        r.sharc.Configure()
        rr = r.reconstruction(*out)
        fg = r.frame_generation(*out)

        def default_ms(generate):
            ms = []
            for f in range(a.frames + 4):
                g.desc.camera["Jitter"] = P.upscaler_jitter(f, render, out)
                gs = S.graphics_settings(*render, spp=4, bounces=8, frame_index=f)
                gs["Denoiser"], gs["IsDIEnabled"] = L.DENOISER_DLSS_RR, 1
                b, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                b.record()
                r.render(gs, di_samples=8, di_reuse=L.di_resampling_settings(), sharc=L.sharc_settings(), reconstruct=rr, post=post, generate=generate)
                e.record(); torch.cuda.synchronize()
                ms.append(b.elapsed_time(e))
            g.desc.camera["Jitter"] = (0.0, 0.0)
            return statistics.median(ms[4:])
        without = [default_ms(None)]
        with_pass = default_ms(fg)
        without.append(default_ms(None))
        ref = min(without)
        emit({"workload": "c2 default configuration", "render": list(render), "output": list(out), "frame_ms_without": round(ref, 4),
              "frame_ms_with": round(with_pass, 4), "pass_ms": round(with_pass - ref, 4), "rendered_fps_without": round(1e3 / ref, 1),
              "rendered_fps_with": round(1e3 / with_pass, 1), "displayed_fps_without": round(1e3 / ref, 1), "displayed_fps_with": round(2e3 / with_pass, 1)})
        g.close()
    ctx.close()


if __name__ == "__main__":
    main()
