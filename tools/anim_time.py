"""Developer helper (GPU): what a dynamic frame's UPDATE costs when the pose comes from keyframes on the device, and what pt_anim_evaluate costs alone.

  A  the update part of bench.py --workload dynamic's frame (pose, skin, refit, top level; no render) on its scene, two ways, each in a context
     of its own, alternating:
       device  Scene.Animate: pt_anim_evaluate (one launch) -> pt_skin_mesh from the device's joint matrices -> pt_update_bottom_level ->
               pt_build_top_level_posed (one more launch than pt_build_top_level: the patch of the posed instances)
       host    what the parent commit had: scenes.bar_pose on the host -> Scene.SkinSkeletalMeshes (pinned staging ring, one copy) ->
               pt_update_bottom_level -> pt_build_top_level
     per way: the time of --frames updates enqueued back to back and ended by ONE synchronise, per update; the host time until the last
     call of such a batch returns, per update (what the host thread pays; nothing in either way waits for the device); and the DEVICE time
     of one update: events around it, the update enqueued while the device is still busy with a filler (a 1 GiB memset, three times), so
     that the interval holds the update's copies and kernels and none of the host's enqueue time.
  B  pt_anim_evaluate alone at 1, 64 and 1024 animated objects sharing one rig of --nodes nodes (each with a rotation channel of 8 keys, one skin
     of --nodes / 2 joints): --calls calls back to back, one synchronise, per call; and the device time of one call, behind the same filler.
Warm-up first; --rounds rounds, the spread of the rounds next to every median. Prints one JSON line per measurement and writes them to --out.
usage: tools/anim_time.py [--rounds 7] [--frames 200] [--calls 200] [--nodes 64] [--out profiles/anim/anim_time.jsonl]"""
import argparse, ctypes as C, json, math, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7); ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--calls", type=int, default=200); ap.add_argument("--nodes", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "anim", "anim_time.jsonl"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import __graft_entry__ as ge
    ge.load_package()
    import dxpbrt_amd.scenes as S, dxpbrt_amd.ptamd as P, dxpbrt_amd.layouts as L
    import torch
    lines = []
    filler = torch.empty(1 << 30, dtype=torch.uint8, device="cuda:0")

    def device_us(enqueue, n=30):
        """the device time of what enqueue() enqueues: median over n, each behind a filler that outlasts the host's enqueue"""
        out = []
        for _ in range(n):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            for _ in range(3):
                filler.zero_()
            s.record(); enqueue(); e.record()
            torch.cuda.synchronize()
            out.append(s.elapsed_time(e) * 1e3)
        return {"median": statistics.median(out), "min": min(out), "max": max(out)}
    spread = lambda v: {"median": statistics.median(v), "min": min(v), "max": max(v)}      # noqa: E731

    # ---- A: the update of the dynamic workload's frame
    lanes = {}
    for way in ("device", "host"):
        sc = S.dynamic_instanced(n=32, aspect=16 / 9)
        if way == "device":
            S.animate_bar(sc)
        ctx = P.DeviceContext(0); ctx.set_sharding(0, 1, 16)
        g = P.Scene(ctx, sc)
        lanes[way] = (ctx, g, sc, P.Animation(ctx, sc.animations) if way == "device" else None)

    def update(way, i):
        ctx, g, sc, anim = lanes[way]
        if way == "device":
            anim.Tick(1.0 / 60.0)
            g.Animate(anim)
        else:
            g.SkinSkeletalMeshes(sc.nodes[-1].meshes[0], S.bar_pose(30.0 * math.sin(0.2 * i), 0.05 * (i % 7)))
            g.UpdateAccelerationStructures(len(sc.nodes) - 1)

    def updates(way, first, n):
        ctx = lanes[way][0]
        ctx.sync(); t0 = time.perf_counter()
        for i in range(first, first + n):
            update(way, i)
        t1 = time.perf_counter(); ctx.sync(); t2 = time.perf_counter()
        return (t2 - t0) / n * 1e6, (t1 - t0) / n * 1e6

    for way in lanes:
        updates(way, 0, 20)
    us = {w: ([], []) for w in lanes}
    for rnd in range(a.rounds):
        for way in ("device", "host", "device", "host"):
            total, host = updates(way, 100 + rnd * a.frames, a.frames)
            us[way][0].append(total); us[way][1].append(host)
    for way in lanes:
        lines.append({"measurement": "dynamic frame update, " + way + "-posed", "scene": "scenes.dynamic_instanced(32): 1027 instances, one skinned 2048-triangle column",
                      "update_us": spread(us[way][0]), "host_enqueue_us": spread(us[way][1]), "device_us": device_us(lambda: update(way, 7)), "updates_per_batch": a.frames, "batches": 2 * a.rounds,
                      "waits_inside_the_update": 0})
    lines.append({"summary": "device-posed minus host-posed update", "update_us": statistics.median(us["device"][0]) - statistics.median(us["host"][0]),
                  "host_enqueue_us": statistics.median(us["device"][1]) - statistics.median(us["host"][1]),
                  "spread_of_one_way_us": max(us["host"][0]) - min(us["host"][0]),
                  "launches_added": "pt_anim_evaluate: 1 kernel + 1 async copy of the states; pt_build_top_level_posed: 1 kernel; removed: the copy of the host matrices"})
    for ctx, g, sc, anim in lanes.values():
        if anim is not None:
            anim.close()
        g.close(); ctx.close()

    # ---- B: pt_anim_evaluate alone
    n = a.nodes
    rng = np.random.default_rng(5)
    parents = [-1] + [int(rng.integers(max(0, k - 8), k)) for k in range(1, n)]
    ident = (0.0, 0.0, 0.0) + (0.0, 0.0, 0.0, 1.0) + (1.0, 1.0, 1.0)
    times = [0.25 * k for k in range(8)]
    clip = {(k, 1): (times, [S.quat_z(float(rng.uniform(-60, 60))) for _ in times]) for k in range(n)}
    rig = S.rig_from_channels(parents, [ident] * n, [clip])
    eye = np.eye(4, dtype=np.float32)
    joints = np.arange(n // 2, dtype=np.uint32)
    for count in (1, 64, 1024):
        ctx = P.DeviceContext(0)
        inst = torch.zeros(count * L.INSTANCE_DATA.itemsize, dtype=torch.uint8, device="cuda:0")
        ctx.check(ctx.lib.pt_set_instance_data(ctx.handle, C.c_void_p(inst.data_ptr()), count))
        objs = [S.AnimatedObject(rig, eye, np.array([n - 1], np.uint32), np.array([k], np.uint32), eye[None], [S.Skin(0, joints, np.stack([eye] * len(joints)))]) for k in range(count)]
        anim = P.Animation(ctx, objs)

        def calls(k):
            ctx.sync(); t0 = time.perf_counter()
            for _ in range(k):
                anim.Tick(1.0 / 60.0)
                anim.Evaluate(inst)
            t1 = time.perf_counter(); ctx.sync()
            return (time.perf_counter() - t0) / k * 1e6, (t1 - t0) / k * 1e6
        calls(20)
        r = [calls(a.calls) for _ in range(a.rounds)]
        lines.append({"measurement": "pt_anim_evaluate alone", "objects": count, "nodes_per_rig": n, "joints_per_object": len(joints), "launches_per_call": 1,
                      "call_us": spread([x[0] for x in r]), "host_enqueue_us": spread([x[1] for x in r]), "device_us": device_us(lambda: anim.Evaluate(inst)), "calls_per_batch": a.calls, "batches": a.rounds})
        anim.close(); ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        for ln in lines:
            print(json.dumps(ln), flush=True)
            fh.write(json.dumps(ln) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
