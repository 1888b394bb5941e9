"""Developer helper: time the direct-lighting pass (HIP events around N back-to-back pt_di_render calls) and one DI-on frame (G-buffer + DI +
path tracer with IsDIEnabled) against the DI-off frame, per workload. Each workload runs in a child process of its own. --reuse also times
the pass with temporal + spatial reservoir reuse at the reference's defaults (layouts.di_resampling_settings), history carried over.
--visibility (with --reuse) adds the pass with visibility in the reservoirs (layouts.di_visibility_settings): initial visibility, + Raytraced in both
passes, + final-visibility reuse, each with the final shadow rays per pixel counted from the downloaded reservoirs (a shaded reservoir
whose visibility has age 0 was traced this frame, an older one was reused). --pairwise (with --reuse) times Basic and Pairwise bias
correction (layouts.di_pairwise_settings, both passes) side by side at SpatialSamples 1 and 4, three alternating rounds each. --light-sampling times each listed local-light sampling mode (cdf, uniform, power_ris, regir, regir_onion: ReGIR over the Onion layout; one JSON line per mode). The workload
--brdf-samples 0,1,2 times the plain pass with that many BRDF candidates per pixel (layouts.di_brdf_settings; 0 is the pass as it was): "brdf": {N_B: pass ms}; the BRDF-ray kernel's own share is the
difference to N_B = 0 less what the candidates add to initial sampling, and `rocprofv3 --kernel-trace --stats -- python tools/di_time.py --child W --brdf-samples 1` names it (k_di_brdf_rays). The workload
emitter_field is scenes.emitter_field(256) (131 k emissive triangles) at 1920 x 1080, 1 spp, 1 bounce. --pdf-mipmap times every listed
--light-sampling mode twice, with the local-light PDF texture off and on (DirectLighting.SetPdfMipmap; "pdf_mipmap" in the JSON line): the
texture and its chain are built in every mode, the descent replaces the prefix sum in power_ris, regir and regir_onion.
usage: tools/di_time.py [--workloads c2,c3,c5,emitter_field] [--samples 8] [--n 20] [--reuse [--visibility] [--pairwise]] [--light-sampling cdf,regir] [--brdf-samples 0,1,2] [--pdf-mipmap]"""
import argparse, json, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(w, samples, n, reuse, modes, visibility=False, pairwise=False, brdf=(), pdf_mipmap=False):
    sys.path.insert(0, ROOT)
    import torch
    import __graft_entry__ as ge
    ge.load_package()
    import dxpbrt_amd.layouts as L, dxpbrt_amd.ptamd as P, dxpbrt_amd.scenes as S
    import bench
    if w == "emitter_field":
        W, H, spp, bounces, ext = 1920, 1080, 1, 1, 0
        scene = S.emitter_field(256, aspect=W / H)
    else:
        kind, W, H, spp, bounces, desc = bench.WORKLOADS[w]
        scene, ext = bench.make_scene(kind, W / H, S)
    ctx = P.DeviceContext(0)
    ctx.set_frames_in_flight(1)
    g = P.Scene(ctx, scene)
    r = P.Renderer(ctx, g, W, H, with_denoiser_outputs=True, di_history=reuse)
    tlas = g.GetTopLevelAccelerationStructure()
    gs = S.graphics_settings(W, H, spp=spp, bounces=bounces, ext_flags=ext)
    ev = lambda: torch.cuda.Event(enable_timing=True)

    def timed(fn, k):
        a, b = ev(), ev()
        a.record()
        for i in range(k):
            fn(i)
        b.record(); torch.cuda.synchronize()
        return a.elapsed_time(b) / k

    r.render(gs)                                               # G-buffer + warm-up
    ctx.sync()
    off_ms = timed(lambda i: r.render(gs), max(3, n // 4))
    cases = [(mode, pdf) for mode in modes for pdf in ((False, True) if pdf_mipmap else (None,))]
    for mode, pdf in cases:
        ls = None if mode == "cdf" else L.di_light_sampling_settings("regir" if mode == "regir_onion" else mode)
        layout = L.di_regir_layout_settings("onion") if mode == "regir_onion" else None
        r.render(gs)
        ctx.sync()
        r.direct_lighting.SetConstants(L.di_settings(W, H, 0, samples, ext_flags=ext))
        r.direct_lighting.SetLightSampling(ls)
        r.direct_lighting.SetReGIRLayout(layout)
        if pdf is not None:
            r.direct_lighting.SetPdfMipmap(pdf)
        lights = r.direct_lighting.light_count()
        for _ in range(3):
            r.direct_lighting.Render(tlas)
        ctx.sync()
        di_ms = timed(lambda i: r.direct_lighting.Render(tlas), n)
        gs_on = gs.copy(); gs_on["IsDIEnabled"] = 1
        r.render(gs_on, di_samples=samples, di_light_sampling=ls, di_regir_layout=layout); ctx.sync()
        on_ms = timed(lambda i: r.render(gs_on, di_samples=samples, di_light_sampling=ls, di_regir_layout=layout), max(3, n // 4))
        out = {"workload": w, "size": [W, H], "lights": lights, "samples": samples, "light_sampling": mode, "di_ms": di_ms,
               "frame_di_off_ms": off_ms, "frame_di_on_ms": on_ms}
        if pdf is not None:
            out["pdf_mipmap"] = pdf
        if (mode, pdf) != cases[-1]:
            print(json.dumps(out), flush=True)
    if pdf_mipmap:
        r.direct_lighting.SetPdfMipmap(False)
    if brdf:                                                   # the plain pass of the last mode with N_B BRDF candidates, alternating twice
        rows = {}
        for rnd in range(2):
            for nb in brdf:
                r.direct_lighting.SetBrdfSampling(L.di_brdf_settings(nb) if nb else None)
                for _ in range(3):
                    r.direct_lighting.Render(tlas)
                ctx.sync()
                rows.setdefault(str(nb), []).append(timed(lambda i: r.direct_lighting.Render(tlas), n))
        r.direct_lighting.SetBrdfSampling(None)
        out["brdf"] = rows
    if reuse:
        r.render(gs, di_samples=samples, di_reuse=L.di_resampling_settings()); ctx.sync()     # Previous* G-buffer, first history
        r.direct_lighting.Render(tlas); ctx.sync()
        out["di_reuse_ms"] = timed(lambda i: r.direct_lighting.Render(tlas), n)

        def final_rays():
            res = r.direct_lighting.download_reservoirs()
            shaded = (res["LightIndex"] != 0xFFFFFFFF) & (res["W"] > 0)
            age = L.di_unpack_visibility(res["Visibility"])[3]
            return float((shaded & (age == 0)).sum()) / (W * H), float((shaded & (age > 0)).sum()) / (W * H)
        out["final_rays_per_pixel"] = final_rays()[0]
        rows = [("initial", L.di_visibility_settings(final_reuse=False)),
                ("initial_raytraced", L.di_visibility_settings(final_reuse=False, temporal_raytraced=True, spatial_raytraced=True)),
                ("initial_raytraced_final_reuse", L.di_visibility_settings(temporal_raytraced=True, spatial_raytraced=True))] if visibility else []
        for label, vs in rows:
            r.direct_lighting.SetVisibility(vs)
            for _ in range(6):                                 # the history refills; stored visibilities reach every age up to MaxAge
                r.direct_lighting.Render(tlas)
            ctx.sync()
            ms = timed(lambda i: r.direct_lighting.Render(tlas), n)
            traced, reused = final_rays()
            out["visibility_" + label] = {"di_reuse_ms": ms, "final_rays_per_pixel": traced, "final_reused_per_pixel": reused}
        r.direct_lighting.SetVisibility(None)
        if pairwise:                                           # Basic against Pairwise, alternating: the spread between rounds is the noise
            rows = {}
            for spatial in (1, 4):
                r.direct_lighting.SetResampling(L.di_resampling_settings(spatial_samples=spatial))
                for rnd in range(3):
                    for label, pw in (("basic", None), ("pairwise", L.di_pairwise_settings(temporal=True, spatial=True))):
                        r.direct_lighting.SetPairwise(pw)
                        for _ in range(6):                     # the history refills up to MaxHistoryLength: no disocclusion boost in the window
                            r.direct_lighting.Render(tlas)
                        ctx.sync()
                        rows.setdefault("%s_spatial%d_ms" % (label, spatial), []).append(timed(lambda i: r.direct_lighting.Render(tlas), n))
            out["pairwise"] = rows
            r.direct_lighting.SetPairwise(None)
        r.direct_lighting.SetResampling(None)
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default=None); ap.add_argument("--workloads", default="c2,c3,c5")
    ap.add_argument("--samples", type=int, default=8); ap.add_argument("--n", type=int, default=20); ap.add_argument("--reuse", action="store_true")
    ap.add_argument("--light-sampling", default="cdf"); ap.add_argument("--visibility", action="store_true")
    ap.add_argument("--pairwise", action="store_true"); ap.add_argument("--brdf-samples", default="")
    ap.add_argument("--pdf-mipmap", action="store_true")
    a = ap.parse_args()
    if a.child:
        child(a.child, a.samples, a.n, a.reuse, a.light_sampling.split(","), a.visibility, a.pairwise,
              [int(v) for v in a.brdf_samples.split(",") if v], a.pdf_mipmap); sys.exit(0)
    for w in a.workloads.split(","):
        p = subprocess.run([sys.executable, __file__, "--child", w, "--samples", str(a.samples), "--n", str(a.n),
                            "--light-sampling", a.light_sampling] + (["--reuse"] if a.reuse else []) + (["--visibility"] if a.visibility else []) +
                           (["--pairwise"] if a.pairwise else []) + (["--brdf-samples", a.brdf_samples] if a.brdf_samples else []) + (["--pdf-mipmap"] if a.pdf_mipmap else []), stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, text=True, timeout=600)
        line = [l for l in p.stdout.splitlines() if l.startswith("{")]
        print("\n".join(line) if line else "%s FAILED (exit %d) %s" % (w, p.returncode, p.stderr[-400:]), flush=True)
        if p.returncode < 0:                                    # a child killed by a signal: start nothing more on the GPU
            sys.exit(1)
