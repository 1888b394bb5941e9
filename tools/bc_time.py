"""Developer helper (GPU): what block-compressed textures buy on the C3 textured frame. Builds scenes.sponza_scale(textured=True) three ways
  a  as bench.py --workload c3t renders it: RGBA8 / RGBA8_SRGB textures
  b  base colour as BC3_SRGB, normals as BC5, metallic-roughness as BC1 (bc.encode: a range-fit encoder, so b is not a's image)
  c  the expansions of b's blocks: RGBA8(_SRGB) for BC3 / BC1, R32G32B32A32_FLOAT for BC5 -- the same image as b, bit for bit
checks that b and c give the same frame bits, then times b against c and a against c in one process, alternating, each variant in a context
of its own: warm-up, --rounds rounds of --frames frames per variant, the spread of the rounds of one variant next to every difference.
Prints one JSON line per variant (frame ms, the k_shade<true> launch mean from the library's events, texture bytes resident) and a summary
line, and writes them to --out.
usage: tools/bc_time.py [--rounds 7] [--frames 12] [--texture-size 1024] [--n-side 354] [--out profiles/bc/bc_time_c3t.jsonl]"""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7); ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--texture-size", type=int, default=1024); ap.add_argument("--n-side", type=int, default=354)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bc", "bc_time_c3t.jsonl"))
    ap.add_argument("--build-only", action="store_true", help="build and encode the three scenes, report the time, touch no GPU")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import __graft_entry__ as ge
    ge.load_package()
    import dxpbrt_amd.bc as bc, dxpbrt_amd.scenes as S
    import bench
    kind, W, H, spp, bounces, desc = bench.WORKLOADS["c3t"]
    fmts = {"BaseColor": S.FMT_BC3_UNORM_SRGB, "Normal": S.FMT_BC5_UNORM, "MetallicRoughness": S.FMT_BC1_UNORM}
    t0 = time.perf_counter()
    make = lambda: S.sponza_scale(n_side=a.n_side, aspect=W / H, textured=True, texture_size=a.texture_size)      # noqa: E731
    cache = {}

    def compress(slot, t):
        return cache.setdefault(len(cache), bc.block_texture(t, fmts[slot]))
    scenes = {"a": make(), "b": bc.map_textures(make(), compress)}
    blocks = iter(list(cache.values()))                  # the same walk over the same scene: c's textures are b's blocks, expanded
    scenes["c"] = bc.map_textures(make(), lambda slot, t: bc.expansion(next(blocks)))
    names = {"a": "rgba8 (bench c3t)", "b": "bc3_srgb + bc5 + bc1", "c": "expansion of b"}
    tex_bytes = {k: int(sum(it.array.nbytes for it in sc.heap if it.kind != S.KIND_BUFFER)) for k, sc in scenes.items()}
    print(f"# scenes built and encoded in {time.perf_counter() - t0:.1f} s; texture bytes {tex_bytes}", flush=True)
    if a.build_only:
        return 0

    import dxpbrt_amd.ptamd as P
    lanes = {}
    for k, sc in scenes.items():
        ctx = P.DeviceContext(0); ctx.set_sharding(0, 1, 16)
        g = P.Scene(ctx, sc)
        lanes[k] = (ctx, g, P.Renderer(ctx, g, W, H, with_f32=True))
    gs = lambda i: S.graphics_settings(W, H, spp=spp, bounces=bounces, frame_index=i)      # noqa: E731

    def frames(k, first, n):
        ctx, g, r = lanes[k]
        ctx.sync(); t = time.perf_counter()
        for i in range(n):
            r.render(gs(first + i))
        ctx.sync()
        return (time.perf_counter() - t) / n * 1e3

    # b and c are the same image: the same frame bits, or the timing below compares two different workloads
    bits = {}
    for k in ("b", "c"):
        ctx, g, r = lanes[k]
        r.render(gs(0)); ctx.sync()
        bits[k] = P.textures_to_numpy({"RadianceF32": r.textures["RadianceF32"]})["RadianceF32"].view(np.uint32).copy()
    same = bool(np.array_equal(bits["b"], bits["c"]))
    print(f"# frame bits of b and c identical: {same}", flush=True)
    if not same:
        print(json.dumps({"error": "b and c differ", "differing_words": int((bits["b"] != bits["c"]).sum())}))
        return 1

    for k in lanes:
        frames(k, 1, 3)                                  # warm-up
    ms = {k: [] for k in lanes}
    for rnd in range(a.rounds):                          # b c a c: c is measured twice per round, its two series give the spread of one variant
        for k in ("b", "c", "a", "c"):
            ms[k].append(frames(k, 100 + rnd * a.frames, a.frames))
    shade = {}
    for k, (ctx, g, r) in lanes.items():                 # the k_shade launch mean from the library's events (event mode: no graph replay)
        ctx.enable_kernel_timing(True)
        for i in range(4):
            r.render(gs(500 + i))
        t = ctx.kernel_timing(); ctx.enable_kernel_timing(False)
        shade[k] = (t["shade_ms"] / max(1, t["shade_launches"]), t["shade_launches"])
    c_even, c_odd = ms["c"][0::2], ms["c"][1::2]
    lines = []
    for k in ("a", "b", "c"):
        lines.append({"variant": k, "textures": names[k], "workload": desc, "frame_ms_median": statistics.median(ms[k]), "frame_ms_min": min(ms[k]),
                      "frame_ms_max": max(ms[k]), "frame_ms_rounds": [round(x, 4) for x in ms[k]], "k_shade_launch_mean_ms": shade[k][0],
                      "k_shade_launches": shade[k][1], "texture_bytes_resident": tex_bytes[k], "rounds": a.rounds, "frames_per_round": a.frames,
                      "texture_size": a.texture_size})
    med = lambda v: statistics.median(v)                 # noqa: E731
    lines.append({"summary": "c3t block compression", "same_frame_bits_b_c": same,
                  "spread_c_ms": {"between_its_two_series": abs(med(c_even) - med(c_odd)), "max_minus_min": max(ms["c"]) - min(ms["c"])},
                  "b_minus_c_frame_ms": med(ms["b"]) - med(ms["c"]), "a_minus_c_frame_ms": med(ms["a"]) - med(ms["c"]),
                  "b_minus_c_k_shade_ms": shade["b"][0] - shade["c"][0], "a_minus_c_k_shade_ms": shade["a"][0] - shade["c"][0]})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        for ln in lines:
            print(json.dumps(ln), flush=True)
            fh.write(json.dumps(ln) + "\n")
    for ctx, g, r in lanes.values():
        g.close(); ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
