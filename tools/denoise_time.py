"""Developer helper: time the denoiser (pt_denoiser_process) at 1920 x 1080 and 3840 x 2160.

A call is 2 + AtrousIterations launches, so the stages are timed as differences of whole calls, each call between two HIP events, median
of --n calls after a warm-up, on a history that is 8 frames long (the variance then comes from the moments; --short-history times the
calls right after a reset instead, where it comes from the 7 x 7 neighbourhood):
    temporal            the call with AtrousIterations = 0
    variance + step 1   the call with 1 iteration minus that
    step 2^k            the call with k + 1 iterations minus the call with k
once with every a-trous step in the direct form (PT_DENOISER_FORM_DIRECT) and once in the staged form (PT_DENOISER_FORM_STAGED: steps 1, 2
and 4; the wider ones are direct in both), alternating. Beside every stage, in the same process, a hipMemcpyAsync device-to-device copy
sized so that it reads and writes as many bytes as the stage must (a copy of n bytes reads n and writes n). Bytes per pixel:
    temporal   52 read (Position 16, LinearDepth 4, NormalRoughness 8, MotionVector 8, the noisy pair 16) + 88 of the last frame's history
               (guides 32, colours 32, moments 16, lengths 8: each texel once, whatever the four taps share) + 88 written (the same arrays of
               this frame) + 16 (the Denoised pair, AtrousIterations = 0 only) = 244
    variance   40 read (moments 16, lengths 8, guide 16) + 8 written = 48 on a long history
    a-trous    72 read (guides 32, colours 32, variance 8: each texel once) + 40 written (16 in the last iteration) = 112
Then a C2 frame (Cornell box, 4 spp, 8 bounces, Denoiser ReLAX, one frame in flight) through render(..., nrd=RELAX) with the identity and
with the denoiser. One JSON line per case, also appended to --out.
usage: tools/denoise_time.py [--sizes 1920x1080,3840x2160] [--n 30] [--frames 10] [--no-c2] [--short-history] [--out profiles/denoise/denoise_time.jsonl]"""
import argparse, ctypes as C, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEBUG_DIRECT, DEBUG_STAGED = 0x800, 0x1000
BYTES = {"temporal": 244, "variance": 48, "atrous": 112}


def hip_runtime():
    """the HIP runtime this process already uses (torch's), for hipMemcpyAsync"""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return C.CDLL(line.split()[-1])
    raise SystemExit("no HIP runtime is loaded")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1920x1080,3840x2160"); ap.add_argument("--n", type=int, default=30)
    ap.add_argument("--frames", type=int, default=10); ap.add_argument("--no-c2", action="store_true")
    ap.add_argument("--short-history", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise", "denoise_time.jsonl"))
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
        raise SystemExit("denoise_time.py measures on the GPU: none is visible")
    ctx = P.DeviceContext(0)
    dev = torch.device("cuda", 0)
    hip = hip_runtime()
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    log = open(a.out, "a")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True); log.write(line + "\n"); log.flush()

    def median_us(fn, n, before=None):
        """each call between two events of its own on the stream the library and the copy use (the null stream)"""
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
        for b, e in ev:
            if before:
                before()
            b.record(); fn(); e.record()
        torch.cuda.synchronize()
        return statistics.median(b.elapsed_time(e) for b, e in ev) * 1e3

    op = P.Denoiser(ctx)
    rng = np.random.default_rng(1)
    for size in a.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        px = W * H
        ys, xs = np.mgrid[0:H, 0:W]
        pos = np.zeros((H, W, 4), np.float32)          # the plane z = 5 seen through a 60-degree lens, facing the camera
        pos[..., 0] = (xs - W / 2) * (5.8 / W); pos[..., 1] = (ys - H / 2) * (5.8 / W); pos[..., 2] = 5.0
        nr = np.zeros((H, W, 4), np.int16); nr[..., 2] = -32767; nr[..., 3] = 16384

        def noisy():
            return torch.from_numpy((1.0 + rng.uniform(-0.5, 0.5, (H, W, 4))).astype(np.float16).view(np.int16)).to(dev)
        tex = {"Position": torch.from_numpy(pos).to(dev), "LinearDepth": torch.full((H, W), 5.0, dtype=torch.float32, device=dev),
               "NormalRoughness": torch.from_numpy(nr).to(dev), "MotionVector": torch.zeros((H, W, 4), dtype=torch.int16, device=dev),
               "NoisyDiffuse": noisy(), "NoisySpecular": noisy()}
        tex["DenoisedDiffuse"], tex["DenoisedSpecular"] = torch.empty_like(tex["NoisyDiffuse"]), torch.empty_like(tex["NoisySpecular"])
        src = torch.empty(122 * px, dtype=torch.uint8, device=dev); dst = torch.empty_like(src)
        call_us = {}
        for k in range(6):
            for form, flag in (("direct", DEBUG_DIRECT), ("staged", DEBUG_STAGED)):
                ctx.set_debug_flags(flag)
                op.SetConstants(L.denoiser_settings(W, H, AtrousIterations=k, MaxAccumulatedFrames=8))   # other settings: the history restarts
                if a.short_history:
                    call_us[(k, form)] = median_us(lambda: op.Process(tex), a.n, before=op.ResetHistory)
                else:
                    for _ in range(8):
                        op.Process(tex)
                    call_us[(k, form)] = median_us(lambda: op.Process(tex), a.n)
        ctx.set_debug_flags(0)

        def copy_us(nbytes):
            return median_us(lambda: hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), nbytes // 2, 3, None), a.n)
        base = {"size": [W, H], "history": "short" if a.short_history else "long", "calls_timed": a.n}
        t0 = min(call_us[(0, "direct")], call_us[(0, "staged")])               # the same launch under either flag
        c = copy_us(BYTES["temporal"] * px)
        emit(dict(base, stage="temporal", B_per_px=BYTES["temporal"], us=round(t0, 2), us_same_bytes_copy=round(c, 2), ratio_to_copy=round(t0 / c, 3),
                  TB_per_s=round(BYTES["temporal"] * px / (t0 * 1e-6) / 1e12, 3)))
        c = copy_us((BYTES["variance"] + BYTES["atrous"]) * px)
        for k in range(1, 6):
            step = 1 << (k - 1)
            us = {f: call_us[(k, f)] - call_us[(k - 1, f)] for f in ("direct", "staged")}
            rec = dict(base, stage=("variance + a-trous step 1" if k == 1 else f"a-trous step {step}"), step=step,
                       B_per_px=BYTES["atrous"] + (BYTES["variance"] if k == 1 else 0), us_direct=round(us["direct"], 2),
                       us_staged=round(us["staged"], 2) if step <= 4 else None, staged_is_direct_at_this_step=step > 4)
            if k == 2:
                c = copy_us(BYTES["atrous"] * px)
            best = min(us["direct"], us["staged"]) if step <= 4 else us["direct"]
            emit(dict(rec, us_same_bytes_copy=round(c, 2), ratio_to_copy=round(best / c, 3), TB_per_s=round(rec["B_per_px"] * px / (best * 1e-6) / 1e12, 3)))
        emit(dict(base, stage="whole call, 5 iterations", us_direct=round(call_us[(5, "direct")], 2), us_staged=round(call_us[(5, "staged")], 2)))
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
                b.record(); r.render(gs, nrd=L.DENOISER_NRD_RELAX, **kw); e.record(); torch.cuda.synchronize()
                ms.append(b.elapsed_time(e))
            return statistics.median(ms)
        r.render(gs, nrd=L.DENOISER_NRD_RELAX, denoise=r.denoiser); r.render(gs, nrd=L.DENOISER_NRD_RELAX); ctx.sync()
        off = frame_ms(); on = frame_ms(denoise=r.denoiser); off2 = frame_ms()
        emit({"workload": "c2", "denoiser": "relax", "size": [W, H], "frame_ms_identity": round(min(off, off2), 4),
              "frame_ms_denoised": round(on, 4), "denoiser_share": round((on - min(off, off2)) / on, 4)})
        g.close()
    ctx.close()


if __name__ == "__main__":
    main()
