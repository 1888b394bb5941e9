"""Developer helper: time pt_mipmap_generate. The full chain of an R32_FLOAT texture at each size, the call between two HIP events, median of
--n calls after a warm-up; beside it, in the same process, a hipMemcpyAsync device-to-device copy that reads and writes as many bytes as
the chain: the chain reads level 0 (the levels a launch re-reads from the one before are a twentieth of it) and writes every other level,
4 * (texels of level 0 + texels of levels 1..) bytes, so the copy moves half of that. The launch count is ceil((mips - 1) / 5). One JSON
line per size, also appended to --out.
usage: tools/mip_time.py [--sizes 32x32,1024x1024,4096x4096] [--n 50] [--out profiles/mip/mip_time.jsonl]"""
import argparse, ctypes as C, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def hip_runtime():
    """the HIP runtime this process already uses (torch's), for hipMemcpyAsync"""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return C.CDLL(line.split()[-1])
    raise SystemExit("no HIP runtime is loaded")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="32x32,1024x1024,4096x4096"); ap.add_argument("--n", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mip", "mip_time.jsonl"))
    a = ap.parse_args()
    if a.n < 20:
        raise SystemExit("--n: the median is taken over at least 20 calls")
    sys.path.insert(0, ROOT)
    import torch
    import __graft_entry__ as ge
    ge.load_package()
    import dxpbrt_amd.ptamd as P
    if not torch.cuda.is_available():
        raise SystemExit("mip_time.py measures on the GPU: none is visible")
    ctx = P.DeviceContext(0)
    dev = torch.device("cuda", 0)
    hip = hip_runtime()
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    log = open(a.out, "a")

    def median_us(fn, n):
        """each call between two events of its own on the stream the library and the copy use (the null stream)"""
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
        for b, e in ev:
            b.record(); fn(); e.record()
        torch.cuda.synchronize()
        return statistics.median(b.elapsed_time(e) for b, e in ev) * 1e3

    op = P.MipmapGeneration(ctx)
    for size in a.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        mips = max(W, H).bit_length()
        levels = [torch.rand((max(1, H >> k), max(1, W >> k)), dtype=torch.float32, device=dev) for k in range(mips)]
        texels = [t.numel() for t in levels]
        nbytes = 4 * (texels[0] + sum(texels[1:]))
        op.SetTexture(levels, W, H)
        us = median_us(op.Process, a.n)
        src = torch.empty(max(nbytes // 2, 4), dtype=torch.uint8, device=dev); dst = torch.empty_like(src)
        copy_us = median_us(lambda: hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), nbytes // 2, 3, None), a.n)
        rec = {"size": [W, H], "mip_levels": mips, "launches": (mips - 1 + 4) // 5, "MB_moved": round(nbytes / 1e6, 3), "us_chain": round(us, 2),
               "calls_timed": a.n, "copy_bytes": nbytes // 2, "us_same_bytes_copy": round(copy_us, 2), "ratio_to_copy": round(us / copy_us, 3),
               "TB_per_s": round(nbytes / (us * 1e-6) / 1e12, 4)}
        line = json.dumps(rec)
        print(line, flush=True); log.write(line + "\n"); log.flush()
    ctx.close()


if __name__ == "__main__":
    main()
