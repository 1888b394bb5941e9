"""Developer helper: time the adaptive sharpener (pt_sharpen_process) and what it costs a frame.

1. The call (one kernel) at 1920x1080 and 3840x2160, between two HIP events, median of --n calls after a warm-up, on a blurred pattern with
   noise (most pixels pass the gate). Beside it, in the same process, a hipMemcpyAsync device-to-device copy of the bytes the call must
   move: 8 B read and 8 B written per pixel, which is what a copy of one frame does.
2. A C2 frame (Cornell box, 4 spp, 8 bounces) rendered at 960 x 540, the upscaler and the post chain at 1920 x 1080, one frame in flight,
   without and with the pass between them.
One JSON line per case, also appended to --out.
usage: tools/sharpen_time.py [--n 30] [--frames 10] [--no-c2] [--out profiles/sharpen/sharpen_time.jsonl]"""
import argparse, ctypes as C, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(1920, 1080), (3840, 2160)]


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sharpen", "sharpen_time.jsonl"))
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
        raise SystemExit("sharpen_time.py measures on the GPU: none is visible")
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

    op = P.Sharpening(ctx)
    rng = np.random.default_rng(1)
    for w, h in CASES:
        y, x = np.mgrid[0:h, 0:w].astype(np.float32)
        img = 0.5 + 0.3 * np.sin(0.3 * x + 0.1 * y)[..., None] * np.cos(0.2 * y)[..., None] + rng.normal(0, 0.02, (h, w, 1)).astype(np.float32)
        color = torch.from_numpy(np.repeat(img, 4, -1).astype(np.float16).view(np.int16)).to(dev)
        tex = {"Color": color, "Sharpened": torch.empty_like(color)}
        nbytes = 16 * w * h                                       # 8 read + 8 written per pixel
        src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev); dst = torch.empty_like(src)
        op.SetConstants(L.sharpen_settings((w, h)))
        us = round(median_us(lambda: op.Process(tex), a.n), 2)
        changed = float((tex["Sharpened"][..., :3] != color[..., :3]).any(-1).float().mean())
        copy = median_us(lambda: hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), nbytes // 2, 3, None), a.n)
        emit({"size": [w, h], "calls_timed": a.n, "bytes": nbytes, "us_call": us, "us_same_bytes_copy": round(copy, 2),
              "ratio_to_copy": round(us / copy, 3), "TB_per_s": round(nbytes / (us * 1e-6) / 1e12, 3), "pixels_changed": round(changed, 3)})
    if not a.no_c2:
        out, render = (1920, 1080), (960, 540)
        ctx.set_frames_in_flight(1)
        g = P.Scene(ctx, S.cornell_box(aspect=out[0] / out[1], variant="ggx"))
        post = L.post_processing_settings(*out)
        r = P.Renderer(ctx, g, *render)
        up = r.upscaler(*out)
        sh = r.sharpening(*out)
        gs = S.graphics_settings(*render, spp=4, bounces=8)

        def frame_ms(sharpen):
            """one frame at a time: the host waits for each"""
            ms = []
            for f in range(a.frames + 2):
                g.desc.camera["Jitter"] = P.upscaler_jitter(f, render, out)
                b, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                b.record(); r.render(gs, post=post, upscale=up, sharpen=sharpen); e.record(); torch.cuda.synchronize()
                ms.append(b.elapsed_time(e))
            g.desc.camera["Jitter"] = (0.0, 0.0)
            return statistics.median(ms[2:])
        without = [frame_ms(None)]
        with_pass = frame_ms(sh)
        without.append(frame_ms(None))
        ref = min(without)
        emit({"workload": "c2", "render": list(render), "output": list(out), "frame_ms_without": round(ref, 4), "frame_ms_with": round(with_pass, 4),
              "pass_ms": round(with_pass - ref, 4), "frame_ms_without_both_runs": [round(v, 4) for v in without]})
        g.close()
    ctx.close()


if __name__ == "__main__":
    main()
