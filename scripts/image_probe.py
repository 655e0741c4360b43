"""Developer tool (GPU box): what the image half of LoadImage::load costs on the device.  Views:
  * 4032 x 3024 RGB to the 1920 cap (1920 x 1440),
  * 3840 x 2160 RGBA with a full-size mask to the cap (1920 x 1080),
  * 1920 x 1080 RGB at LOD image scales 0.5 and 0.25.
Two runs.  First the kernels alone, under the kernel tracer:
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python scripts/image_probe.py --kernels-only
Then the timings, reading DIR for the kernels:
    python scripts/image_probe.py --trace-dir DIR [--reps 20] [--out FILE]
One JSON line per view:
  * kernel_ms: the two resampling passes of bh_resize_u8 on a device-resident image of the view's shape (RGBA for the masked view;
    its mask merge is not included), median dispatch durations from the trace, summed; hbm_gbs: the bytes the passes move (source,
    the f32 intermediate written and read, the output) over that time;
  * call_ms: bh_resize_u8 between ctx-stream events, the weight tables already cached: their copy to pinned memory and to the
    device, and the two kernels;
  * ring_ms: BatchUploader.submit_view -> acquire -> synchronise on the host clock, median: the memcpy into the pinned slot, the
    H2D copy, mask merge, resampling and pack (tables cached after the first view); plain_ms: submit of the same view at full
    size, no resampling.
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import brush_amd as ba   # noqa: E402

VIEWS = [  # name, w, h, channels, mask, max_resolution, scale
    ("4032x3024_rgb_cap1920", 4032, 3024, 3, False, 1920, 1.0),
    ("3840x2160_rgba_mask_cap1920", 3840, 2160, 4, True, 1920, 1.0),
    ("1920x1080_rgb_lod0.5", 1920, 1080, 3, False, 1920, 0.5),
    ("1920x1080_rgb_lod0.25", 1920, 1080, 3, False, 1920, 0.25),
]


def trace_kernel_ms(trace_dir, w, h, nw, nh):
    """Median durations (ms) of the vertical and horizontal pass of a w x h -> nw x nh resize, from kernel_trace.csv files."""
    ver, hor = [], []
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            for r in csv.DictReader(f):
                name, gy = r.get("Kernel_Name", ""), int(r.get("Grid_Size_Y", "0") or 0)
                gx = int(r.get("Grid_Size_X", "0") or 0)
                dt = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6
                if gy != nh:
                    continue
                if "resize_vertical_kernel" in name and gx in ((w + 255) // 256 * 256, (w + 255) // 256):
                    ver.append(dt)
                elif "resize_horizontal_kernel" in name and gx in ((nw + 255) // 256 * 256, (nw + 255) // 256):
                    hor.append(dt)
    if not ver or not hor:
        return None
    return statistics.median(ver) + statistics.median(hor)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernels-only", action="store_true", help="only the bh_resize_u8 calls (run under the kernel tracer)")
    ap.add_argument("--trace-dir", default=None, help="where the --kernels-only run's kernel trace is")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    rng = np.random.default_rng(0)
    rows = []
    for name, w, h, c, masked, mx, scale in VIEWS:
        nw, nh = ba.view_output_size(w, h, mx, scale)
        img = rng.integers(0, 256, (h, w, c), dtype=np.uint8)
        mask = rng.integers(0, 256, (h, w), dtype=np.uint8) if masked else None
        # kernels: resampling of a device-resident image of the same shape
        cr = 4 if masked else c
        src = torch.from_numpy(rng.integers(0, 256, (h, w, cr), dtype=np.uint8)).to(dev)
        out = torch.empty((nh, nw, cr), dtype=torch.uint8, device=dev)
        ctx = ba.get_context(dev)
        lib = ctx.lib
        ks = []
        for r in range(a.reps + 2):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ctx.check(lib.bh_resize_u8(ctx._h, ba.host._ptr(src), w, h, cr, ba.host._ptr(out), nw, nh, 0))
            e1.record()
            e1.synchronize()
            if r >= 2:
                ks.append(e0.elapsed_time(e1))
        call_ms = statistics.median(ks)
        moved = w * h * cr + 2 * w * nh * cr * 4 + nw * nh * cr
        if a.kernels_only:
            print(json.dumps({"view": name, "call_ms": round(call_ms, 4)}), flush=True)
            continue
        kernel_ms = trace_kernel_ms(a.trace_dir, w, h, nw, nh) if a.trace_dir else None
        # the ring, end to end
        staged = img.size + (mask.size if masked else 0)
        up = ba.BatchUploader(max(w * h, (staged + 3) // 4), slots=2)
        ring, plain = [], []
        for r in range(a.reps + 2):
            t0 = time.perf_counter()
            slot = up.submit_view(img, mask=mask, max_resolution=mx, scale=scale)
            packed, _ = up.acquire(slot)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            assert tuple(packed.shape) == (nh, nw)
            up.release(slot)
            t2 = time.perf_counter()
            slot = up.submit(img)
            up.acquire(slot)
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            up.release(slot)
            if r >= 2:
                ring.append((t1 - t0) * 1e3)
                plain.append((t3 - t2) * 1e3)
        up.close()
        torch.cuda.synchronize()
        row = {"view": name, "out": [nw, nh], "kernel_ms": round(kernel_ms, 4) if kernel_ms else "unmeasured",
               "hbm_gbs": round(moved / kernel_ms / 1e6, 1) if kernel_ms else "unmeasured", "kernel_bytes": moved,
               "call_ms": round(call_ms, 4), "ring_ms": round(statistics.median(ring), 3), "plain_ms": round(statistics.median(plain), 3),
               "h2d_bytes": staged, "reps": a.reps}
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
