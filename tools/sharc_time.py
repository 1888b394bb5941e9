"""Developer helper: time the SHARC radiance cache per workload (HIP events on the context's stream). Per workload, in a child process of its
own: the plain frame (G-buffer + path tracer), the frame through the cache at frame 1 (cold cache) and at frame 32 (warm), and the three
passes of the cached frame apart -- update + resolve (a frame with Bounces' query skipped is not available, so they are timed as the frame
with the cache minus a frame whose update and resolve are skipped [PT_DEBUG_SHARC_SKIP_UPDATE, same warm cache]) and the query (that
skipped-update frame minus the G-buffer pass). Secondary rays come from the counters, the update pass's included.
usage: tools/sharc_time.py [--workloads c2,c3,c5] [--n 8] [--downscale 4] [--scene-scale 50]"""
import argparse, json, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(w, n, downscale, scene_scale):
    sys.path.insert(0, ROOT)
    import torch
    import __graft_entry__ as ge
    ge.load_package()
    import dxpbrt_amd.layouts as L, dxpbrt_amd.ptamd as P, dxpbrt_amd.scenes as S
    import bench
    kind, W, H, spp, bounces, desc = bench.WORKLOADS[w]
    scene, ext = bench.make_scene(kind, W / H, S)
    ctx = P.DeviceContext(0)
    ctx.set_frames_in_flight(1)
    g = P.Scene(ctx, scene)
    r = P.Renderer(ctx, g, W, H)
    r.sharc.Configure(0)
    ss = L.sharc_settings(downscale=downscale, scene_scale=scene_scale)
    tlas = g.GetTopLevelAccelerationStructure()
    ev = lambda: torch.cuda.Event(enable_timing=True)
    frame = [100]

    def gs():
        frame[0] += 1
        return S.graphics_settings(W, H, spp=spp, bounces=bounces, frame_index=frame[0], ext_flags=ext)

    def timed(fn, k):
        a, b = ev(), ev()
        a.record()
        for i in range(k):
            fn()
        b.record(); torch.cuda.synchronize()
        return a.elapsed_time(b) / k

    def rays(fn):
        ctx.reset_counters(); fn(); ctx.sync()
        return int(ctx.counters().SecondaryRays)

    r.render(gs()); ctx.sync()                                   # warm-up: allocations, graph capture
    plain_ms = timed(lambda: r.render(gs()), n)
    plain_rays = rays(lambda: r.render(gs()))
    gbuffer_ms = timed(lambda: r.gbuffer.Render(tlas, r.constants), n)
    r.render(gs(), sharc=ss); ctx.sync(); r.sharc.Reset(); ctx.sync()   # the cached frame's allocations and graph, then an empty cache again
    first_ms = timed(lambda: r.render(gs(), sharc=ss), 1)       # frame 1: cold cache
    for _ in range(30):
        r.render(gs(), sharc=ss)
    ctx.sync()
    warm_ms = timed(lambda: r.render(gs(), sharc=ss), n)        # frames 32..: warm
    warm_rays = rays(lambda: r.render(gs(), sharc=ss))
    entries = len(r.sharc.download())
    ctx.set_debug_flags(L.DEBUG_SHARC_SKIP_UPDATE)
    r.render(gs(), sharc=ss); ctx.sync()
    query_frame_ms = timed(lambda: r.render(gs(), sharc=ss), n)
    query_rays = rays(lambda: r.render(gs(), sharc=ss))
    ctx.set_debug_flags(0)
    print(json.dumps({"workload": w, "size": [W, H], "spp": spp, "bounces": bounces, "downscale": downscale, "scene_scale": scene_scale,
                      "frame_plain_ms": plain_ms, "frame_sharc_frame1_ms": first_ms, "frame_sharc_frame32_ms": warm_ms,
                      "gbuffer_ms": gbuffer_ms, "update_resolve_ms": warm_ms - query_frame_ms, "query_ms": query_frame_ms - gbuffer_ms,
                      "path_tracer_plain_ms": plain_ms - gbuffer_ms,
                      "secondary_rays_plain": plain_rays, "secondary_rays_sharc": warm_rays, "secondary_rays_update": warm_rays - query_rays,
                      "live_entries": entries}))
    ctx.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default=None); ap.add_argument("--workloads", default="c2,c3,c5")
    ap.add_argument("--n", type=int, default=8); ap.add_argument("--downscale", type=int, default=4); ap.add_argument("--scene-scale", type=float, default=50.0)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.n, a.downscale, a.scene_scale); sys.exit(0)
    for w in a.workloads.split(","):
        p = subprocess.run([sys.executable, __file__, "--child", w, "--n", str(a.n), "--downscale", str(a.downscale), "--scene-scale", str(a.scene_scale)],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
        line = [l for l in p.stdout.splitlines() if l.startswith("{")]
        print("\n".join(line) if line else "%s FAILED (exit %d) %s" % (w, p.returncode, p.stderr[-400:]), flush=True)
        if p.returncode != 0:                                   # a child that failed, on a signal or on an error: start nothing more on the GPU
            sys.exit(1)
