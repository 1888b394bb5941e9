"""Developer helper: time the post-processing chain (HIP events around N warm back-to-back pt_post_render calls) at 1920 x 1080 and
3840 x 2160, bloom on / off, SDR (ACES filmic) / HDR10, and a C2 frame (Cornell box, 4 spp, 8 bounces, one frame in flight) with and
without the chain. Prints one JSON line per configuration: time per call, launches, the bytes the algorithm must move (every level and
texture read once and written once) and their rate as a share of the 6.29 TB/s measured HBM copy rate. Per-kernel times come from a
separate `rocprofv3 --kernel-trace --stats -- python tools/post_time.py --n 20` run.
usage: tools/post_time.py [--sizes 1920x1080,3840x2160] [--n 100] [--frames 10] [--no-c2]"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_BYTES_PER_S = 6.29e12          # float4 copy, measured on one MI355X


def algorithmic_bytes(W, H, bloom):
    """bytes the chain has to move: Radiance read (twice with bloom: stage 0 and the merge), each bloom level written once and read once by
    the next stage, stage 8's image read by the resolve, Color (8 B) + BackBuffer (4 B) + Display8 (4 B) written"""
    px = W * H
    total = px * 8 + px * 16
    if bloom:
        mips = [(max(1, (W // 2) >> k), max(1, (H // 2) >> k)) for k in range(5)]
        stage_out = [mips[k if k < 5 else 8 - k] for k in range(9)]
        total += px * 8 + sum(2 * w * h * 8 for w, h in stage_out)
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1920x1080,3840x2160"); ap.add_argument("--n", type=int, default=100)
    ap.add_argument("--frames", type=int, default=10); ap.add_argument("--no-c2", action="store_true")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    import __graft_entry__ as ge
    ge.load_package()
    import dxpbrt_amd.layouts as L, dxpbrt_amd.ptamd as P, dxpbrt_amd.scenes as S
    import postref as R
    if not torch.cuda.is_available():
        raise SystemExit("post_time.py measures on the GPU: none is visible")
    ctx = P.DeviceContext(0)
    dev = torch.device("cuda", 0)
    ev = lambda: torch.cuda.Event(enable_timing=True)

    def timed(fn, k):
        b, e = ev(), ev()
        b.record()
        for _ in range(k):
            fn()
        e.record(); torch.cuda.synchronize()
        return b.elapsed_time(e) / k

    op = P.PostProcessing(ctx)
    for size in a.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        rad = torch.from_numpy(R.make_frame(W, H, seed=1, specials=False).view(np.int16).copy()).to(dev)
        tex = dict(P.alloc_post_textures(W, H, dev), Radiance=rad)
        for bloom in (True, False):
            for hdr in (False, True):
                op.SetConstants(L.post_processing_settings(W, H, bloom=bloom, hdr=hdr))
                for _ in range(5):
                    op.Render(tex)
                ctx.sync()
                ms = timed(lambda: op.Render(tex), a.n)
                nbytes = algorithmic_bytes(W, H, bloom)
                print(json.dumps({"size": [W, H], "bloom": bloom, "hdr": hdr, "us_per_call": round(ms * 1e3, 2), "launches": 10 if bloom else 1,
                                  "algorithmic_MB": round(nbytes / 1e6, 2), "TB_per_s": round(nbytes / (ms * 1e-3) / 1e12, 3),
                                  "share_of_hbm": round(nbytes / (ms * 1e-3) / HBM_BYTES_PER_S, 3)}), flush=True)
    if not a.no_c2:
        W, H = 1920, 1080
        ctx.set_frames_in_flight(1)
        g = P.Scene(ctx, S.cornell_box(aspect=W / H, variant="ggx"))
        r = P.Renderer(ctx, g, W, H)
        gs = S.graphics_settings(W, H, spp=4, bounces=8)
        post = L.post_processing_settings(W, H)
        r.render(gs, post=post); r.render(gs); ctx.sync()
        off = timed(lambda: r.render(gs), a.frames)
        on = timed(lambda: r.render(gs, post=post), a.frames)
        off2 = timed(lambda: r.render(gs), a.frames)
        print(json.dumps({"workload": "c2", "size": [W, H], "frame_ms_without_chain": round(min(off, off2), 4),
                          "frame_ms_with_chain": round(on, 4), "chain_share": round((on - min(off, off2)) / on, 4)}), flush=True)
        g.close()
    ctx.close()


if __name__ == "__main__":
    main()
