"""Developer tool (GPU box): what a PLY export costs, uncompressed (bh_splat_to_ply) against compressed
(bh_splat_to_compressed_ply), at 1 M / SH 0, 1 M / SH 3 and 6 M / SH 3 splats of a random scene built on the device.
Prints per configuration, in one process:
  * each call end to end (header, kernels, D2H into a pageable host buffer, the final synchronise) in ms: device events on the
    ctx stream around the call, and the host clock;
  * a plain D2H copy of the same number of bytes (device -> pageable host), the copy's share of the call;
  * the file sizes.
Kernel times come from a separate run under `rocprofv3 --kernel-trace --stats -- python scripts/ply_probe.py --reps 3`.
    python scripts/ply_probe.py [--reps 10] [--sizes 1000000:0,1000000:3,6000000:3]
"""
import argparse
import ctypes as C
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import brush_amd as ba   # noqa: E402
from brush_amd import host   # noqa: E402


def scene(n, deg, dev, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    c = (deg + 1) ** 2
    t = torch.empty((n, 10), device=dev)
    t[:, 0:3] = torch.rand((n, 3), device=dev, generator=g) * 20 - 10
    t[:, 3:7] = torch.randn((n, 4), device=dev, generator=g)
    t[:, 7:10] = torch.rand((n, 3), device=dev, generator=g) * 5 - 7
    sh = torch.rand((n, c, 3), device=dev, generator=g) * 2 - 1
    o = torch.randn((n,), device=dev, generator=g) * 2
    return ba.Splats(t, sh, o, device=dev)


def time_call(fn, reps):
    fn()
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    dev_ms, host_ms = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        host_ms.append((time.perf_counter() - t0) * 1e3)
        dev_ms.append(e0.elapsed_time(e1))
    dev_ms.sort()
    host_ms.sort()
    return dev_ms[len(dev_ms) // 2], host_ms[len(host_ms) // 2], dev_ms[0]


def d2h_ms(nbytes, dev, reps):
    src = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    dst = (C.c_char * nbytes)()
    ptr = C.cast(dst, C.c_void_p).value
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]

    def copy():
        assert hip.hipMemcpy(C.c_void_p(ptr), C.c_void_p(src.data_ptr()), nbytes, 2) == 0   # hipMemcpyDeviceToHost
    return time_call(copy, reps)[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sizes", default="1000000:0,1000000:3,6000000:3")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ctx = ba.get_context(dev)
    print("%-14s %-12s %10s %10s %10s %12s %10s" % ("config", "export", "dev ms", "host ms", "min ms", "bytes", "D2H ms"))
    for spec in a.sizes.split(","):
        n, deg = (int(v) for v in spec.split(":"))
        s = scene(n, deg, dev, 17)
        for name, fn in (("ply", lambda: ba.splat_to_ply(s, ctx=ctx)), ("compressed", lambda: ba.splat_to_compressed_ply(s, ctx=ctx))):
            size = len(fn())
            dm, hm, mn = time_call(fn, a.reps)
            cp = d2h_ms(size, dev, a.reps)
            print("%-14s %-12s %10.2f %10.2f %10.2f %12d %10.2f" % ("%dM/SH%d" % (n // 1000000, deg), name, dm, hm, mn, size, cp), flush=True)
        del s
        torch.cuda.empty_cache()
    host.get_context(dev).sync()


if __name__ == "__main__":
    main()
