"""Developer helper: time the ray-reconstruction pass (pt_reconstruction_process), the chain of existing passes nearest to it, and a C2
frame in the reference's default configuration.

1. The pass at 960x540 -> 1920x1080, 1280x720 -> 1920x1080, 1920x1080 -> 3840x2160 and 1920x1080 native. A call is 3 + AtrousIterations
   launches, so the stages are timed as differences of whole calls, each call between two HIP events, median of --n calls after a warm-up,
   on a history that is 8 frames long with the jitter advancing:
       temporal + variance + resolve   the call with AtrousIterations = 0 (the three launches no setting takes out)
       step 2^k                        the call with k + 1 iterations minus the call with k
   once with every a-trous step in the direct form (PT_RECONSTRUCTION_FORM_DIRECT) and once in the staged form
   (PT_RECONSTRUCTION_FORM_STAGED: steps 1, 2 and 4; the wider ones are direct in both). Beside every stage, in the same process, a
   hipMemcpyAsync device-to-device copy sized so that it reads and writes as many bytes as the stage must (a copy of n bytes reads n and
   writes n). Bytes:
       temporal   per render pixel 60 read (Radiance 8, the albedos 16, NormalRoughness 8, Position 16, LinearDepth 4, MotionVector 8) + 56
                  of the last frame's history (signal and length 16, moments 8, guides 32: each texel once) + 72 written (the same arrays
                  and the albedo 16) = 188
       variance   per render pixel 40 read (signal 16, moments 8, guide 16) + 16 written = 56 on a long history
       resolve    per render pixel 44 read (filtered 16, albedo 16, LinearDepth 4, MotionVector 8); per output pixel 20 of the last output
                  history read, 20 written, 8 of Color = 48
       a-trous    per render pixel 48 read (guides 32, signal and variance 16) + 16 written = 64
   Also the call right after a reset with 5 iterations, where the variance comes from the 7 x 7 walk.
2. The parent's nearest equivalent through the existing entry points on the same sizes, each call between two events: the NRD pack,
   pt_denoiser_process (5 iterations, the form the library chooses), the NRD compose, pt_upscaler_process.
3. A C2 frame (Cornell box, 4 spp, 8 bounces, one frame in flight) in the default configuration at 960 x 540: radiance cache, ReSTIR DI,
   Denoiser = DLSS-RR, reconstruction to 1920 x 1080, post; beside the same frame without the reconstruction and the post chain at
   960 x 540.
One JSON line per case, also appended to --out.
usage: tools/reconstruct_time.py [--n 30] [--frames 10] [--no-c2] [--out profiles/reconstruct/reconstruct_time.jsonl]"""
import argparse, ctypes as C, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEBUG_DIRECT, DEBUG_STAGED = 0x8000, 0x10000
CASES = [((960, 540), (1920, 1080)), ((1280, 720), (1920, 1080)), ((1920, 1080), (3840, 2160)), ((1920, 1080), (1920, 1080))]
RENDER_BYTES = {"frame": 188 + 56 + 44, "atrous": 64}
OUTPUT_BYTES = 48


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reconstruct", "reconstruct_time.jsonl"))
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
        raise SystemExit("reconstruct_time.py measures on the GPU: none is visible")
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
            if before:
                before()
            fn()
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
        for b, e in ev:
            if before:
                before()
            b.record(); fn(); e.record()
        torch.cuda.synchronize()
        return statistics.median(b.elapsed_time(e) for b, e in ev) * 1e3

    op, dn, up, nrd = P.Reconstruction(ctx), P.Denoiser(ctx), P.Upscaler(ctx), P.NRDComposition(ctx)
    rng = np.random.default_rng(1)
    for render, output in CASES:
        (W, H), (Ow, Oh) = render, output
        px, opx = W * H, Ow * Oh
        ys, xs = np.mgrid[0:H, 0:W]
        pos = np.zeros((H, W, 4), np.float32)          # the plane z = 5 seen through a 60-degree lens, facing the camera
        pos[..., 0] = (xs - W / 2) * (5.8 / W); pos[..., 1] = (ys - H / 2) * (5.8 / W); pos[..., 2] = 5.0
        nr = np.zeros((H, W, 4), np.int16); nr[..., 2] = -32767; nr[..., 3] = 16384

        def half(lo, hi):
            return torch.from_numpy(rng.uniform(lo, hi, (H, W, 4)).astype(np.float16).view(np.int16)).to(dev)
        tex = {"Position": torch.from_numpy(pos).to(dev), "LinearDepth": torch.full((H, W), 5.0, dtype=torch.float32, device=dev),
               "NormalRoughness": torch.from_numpy(nr).to(dev), "MotionVector": torch.zeros((H, W, 4), dtype=torch.int16, device=dev),
               "Radiance": half(0.5, 1.5), "DiffuseAlbedo": half(0.2, 0.8), "SpecularAlbedo": half(0.0, 0.2),
               "Color": torch.empty((Oh, Ow, 4), dtype=torch.int16, device=dev)}
        nbytes_max = RENDER_BYTES["frame"] * px + OUTPUT_BYTES * opx
        src = torch.empty(nbytes_max // 2 + 8, dtype=torch.uint8, device=dev); dst = torch.empty_like(src)
        jitters = [P.upscaler_jitter(f, render, output) for f in range(64)]
        state = {"f": 0}

        def call():
            op.Process(jitters[state["f"] % len(jitters)], tex)
            state["f"] += 1

        def copy_us(nbytes):
            return median_us(lambda: hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), nbytes // 2, 3, None), a.n)
        call_us = {}
        for k in range(6):
            for form, flag in (("direct", DEBUG_DIRECT), ("staged", DEBUG_STAGED)):
                ctx.set_debug_flags(flag)
                op.SetConstants(L.reconstruction_settings(render, output, AtrousIterations=k, MaxAccumulatedFrames=8, MaxOutputFrames=8))   # other settings: the history restarts
                for _ in range(8):
                    call()
                call_us[(k, form)] = median_us(call, a.n)
        after_reset = {}
        for form, flag in (("direct", DEBUG_DIRECT), ("staged", DEBUG_STAGED)):
            ctx.set_debug_flags(flag)
            after_reset[form] = median_us(call, a.n, before=op.ResetHistory)
        ctx.set_debug_flags(0)
        base = {"render": list(render), "output": list(output), "calls_timed": a.n}
        t0 = min(call_us[(0, "direct")], call_us[(0, "staged")])               # the same launches under either flag
        nbytes = RENDER_BYTES["frame"] * px + OUTPUT_BYTES * opx
        c = copy_us(nbytes)
        emit(dict(base, stage="temporal + variance + resolve", bytes=nbytes, us=round(t0, 2), us_same_bytes_copy=round(c, 2),
                  ratio_to_copy=round(t0 / c, 3), TB_per_s=round(nbytes / (t0 * 1e-6) / 1e12, 3)))
        nbytes = RENDER_BYTES["atrous"] * px
        c = copy_us(nbytes)
        for k in range(1, 6):
            step = 1 << (k - 1)
            us = {f: call_us[(k, f)] - call_us[(k - 1, f)] for f in ("direct", "staged")}
            best = min(us["direct"], us["staged"]) if step <= 4 else us["direct"]
            emit(dict(base, stage=f"a-trous step {step}", step=step, bytes=nbytes, us_direct=round(us["direct"], 2),
                      us_staged=round(us["staged"], 2) if step <= 4 else None, staged_is_direct_at_this_step=step > 4,
                      us_same_bytes_copy=round(c, 2), ratio_to_copy=round(best / c, 3), TB_per_s=round(nbytes / (best * 1e-6) / 1e12, 3)))
        emit(dict(base, stage="whole call, 5 iterations", us_direct=round(call_us[(5, "direct")], 2), us_staged=round(call_us[(5, "staged")], 2),
                  us_direct_after_reset=round(after_reset["direct"], 2), us_staged_after_reset=round(after_reset["staged"], 2),
                  history_B_per_render_px=160, history_B_per_output_px=40))

        # the parent's nearest equivalent: pack, the two-channel denoiser, compose, the upscaler
        chain = dict(tex, NoisyDiffuse=half(0.5, 1.5), NoisySpecular=half(0.0, 0.5))
        chain["DenoisedDiffuse"], chain["DenoisedSpecular"] = chain["NoisyDiffuse"], chain["NoisySpecular"]
        pack, compose = (L.nrd_composition_constants(W, H, L.DENOISER_NRD_RELAX, p) for p in (True, False))
        dn.SetConstants(L.denoiser_settings(W, H, MaxAccumulatedFrames=8))
        up.SetConstants(L.upscaler_settings(render, output, MaxAccumulatedFrames=8))

        def parent():
            nrd.Process(chain, pack)
            dn.Process(chain)
            nrd.Process(chain, compose)
            up.Process(jitters[state["f"] % len(jitters)], chain)
            state["f"] += 1
        for _ in range(8):
            parent()
        parent_us = median_us(parent, a.n)
        ours = min(call_us[(5, "direct")], call_us[(5, "staged")])
        emit(dict(base, stage="the four-call chain: pack + pt_denoiser_process + compose + pt_upscaler_process", us=round(parent_us, 2),
                  us_reconstruction=round(ours, 2), ratio=round(ours / parent_us, 3)))
        dn.ResetHistory(); up.ResetHistory(); op.ResetHistory()
    if not a.no_c2:
        render, out = (960, 540), (1920, 1080)
        ctx.set_frames_in_flight(1)
        g = P.Scene(ctx, S.cornell_box(aspect=out[0] / out[1], variant="ggx"))
        r = P.Renderer(ctx, g, *render, with_denoiser_outputs=True, di_history=True)
        r.sharc.Configure()
        rr = r.reconstruction(*out)

        def frame_ms(reconstruct):
            """one frame at a time: the host waits for each"""
            ms = []
            for f in range(a.frames + 4):
                g.desc.camera["Jitter"] = P.upscaler_jitter(f, render, out)
                gs = S.graphics_settings(*render, spp=4, bounces=8, frame_index=f)
                gs["Denoiser"], gs["IsDIEnabled"] = L.DENOISER_DLSS_RR, 1
                kw = dict(reconstruct=rr, post=L.post_processing_settings(*out)) if reconstruct else dict(post=L.post_processing_settings(*render))
                b, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                b.record()
                r.render(gs, di_samples=8, di_reuse=L.di_resampling_settings(), sharc=L.sharc_settings(), **kw)
                e.record(); torch.cuda.synchronize()
                ms.append(b.elapsed_time(e))
            g.desc.camera["Jitter"] = (0.0, 0.0)
            return statistics.median(ms[4:])
        on = frame_ms(True); off = frame_ms(False); on2 = frame_ms(True)
        emit({"workload": "c2 default configuration", "render": list(render), "output": list(out), "frame_ms_reconstructed": round(min(on, on2), 4),
              "frame_ms_render_size_post_only": round(off, 4), "reconstruction_and_output_size_post_ms": round(min(on, on2) - off, 4)})
        g.close()
    ctx.close()


if __name__ == "__main__":
    main()
