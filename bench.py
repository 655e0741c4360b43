#!/usr/bin/env python
"""bench.py — headline benchmark of the hot path on MI355X.

A "step" is one SplatTrainer.step (forward render -> L1+SSIM loss -> backward ->
statistics -> Adam + the visibility-gated mean noise, background jittered: the reference's
default step, train.rs:176-429) on ONE 1920x1080 view of the 1 M-splat synthetic scene
(BASELINE.json configs[2]), inputs already resident in HBM.  The timed loop is the
reference's own training bench (crates/brush-bench-test/src/benches.rs:198-220): TWO views, the
second camera 2 units to the right, step k trains view k % 2 (--views V for other counts); every
batch carries its view id, as a loader's batches do.  --windows (3) windows of --steps steps are
timed, each bracketed by barrier + synchronize; the line reports the median window.

--gpus N: data parallel over cameras, one rank per GPU, gradients all-reduced over RCCL between
backward and Adam (weak scaling).  Started either by `python -m torch.distributed.run ... bench.py
--gpus N` (RANK / WORLD_SIZE in the environment) or plainly as `python bench.py --gpus N`, in which
case this process re-executes itself through torch.distributed.run with N ranks on 127.0.0.1.  It
fails loudly when fewer than N devices are visible: it never prints an N=1 line for an N>1 request.

Prints ONE JSON line on rank 0 (contract: see the task statement).  A plain run does what that line's headline needs and nothing
else: it sets up, warms up, times the windows, writes --dump-outputs and prints metric / value / unit / ms_per_step and the
description of what was timed.  --full adds everything else, including
  roofline      — dominant kernel (rasterize_backward_kernel) against HBM: the bytes the launch actually
                  touches / its average duration measured with HIP events on the ctx stream
  roofline_valu — the same kernel (and the forward blend) against the VALU issue rate, which is what bounds them
  stages        — the per-stage table (kernel timestamps of rocprofv3 child runs, or HIP events around each stage)
  cpu_baseline  — the CPU oracle (a C++ restatement of Brush's kernels; Brush has no CPU backend) timed on the
                  host cores on full steps of the same workload
  non_saturating — a second, non-headline measurement on a scene whose tiles do not saturate early
and the training loop, the other view counts, SH degree 3, the object-centric frame, the forward-only render, and with
N > 1 ranks the exchange stages and the exchange A/B.  The N > 1 self-check of the exchange path runs in either mode: it
decides which path is timed.
"""
import argparse
import gc
import json
import math
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md); ~6300 measured achievable
# VALU issue peak: 256 CUs x 4 SIMDs, one wave64 VALU instruction per 2 cycles per SIMD (MI355X_MICROARCH.md:
# "v_fma_f32 (wave64): 2 cyc"), 2.4 GHz -> 1228.8 G wave-instructions/s (full-rate ops; half-rate ops count double)
VALU_PEAK_GINST = 256 * 4 * 2.4 / 2.0
# rasterize_backward_kernel issues this many VALU instructions per blended (splat, tile) — SQ_INSTS_VALU / I_blended,
# profiles/*_sq_counters.csv when present, else this static count from the ISA dump (profiles/*_isa_histogram.txt)
VALU_PER_ISECT_STATIC = {"rasterize_backward_kernel": 249.4, "rasterize_kernel": 103.8}   # profiles/r2f_sq_counters.csv

# stages whose working set the previous kernel left in the 256 MB Infinity Cache: their GB/s is not an HBM rate
CACHE_RESIDENT = {"ProjectBackwards": "reads v_combined (cleared by K5, accumulated by K17) / writes gradient rows the update reads next: still in the 256 MB Infinity Cache",
                  "OptimizerStep": "reads the gradient span the backward just wrote (Infinity-Cache resident at SH degree 0)"}


def stage_bytes(n, nv, ni, ni_blended, pixels, tiles, coeffs, list_share=1.0, grads_cleared=True):
    """HBM bytes per stage: algorithmic (SURVEY.md §8d / DESIGN.md §5), except (i) the two blend kernels, which are charged
    only for the intersections they consume before every pixel of a tile saturates, and (ii) what the depth-sliced lists do not
    list: K5 / tile sort / offsets are charged for the near slice's pairs (list_share of ni; its splats taken as the same share
    of nv).  grads_cleared: the step zero-fills its whole gradient span (the multi-GPU exchange paths) instead of the refine-weight
    vector alone (one GPU)."""
    c = coeffs
    ni_l = int(round(ni * list_share))
    nv_l = int(round(nv * list_share))
    return {
        # K1 also stores the projected record by splat id and clears visible + (part of) the train step's gradient span on its way
        "ProjectSplats": 44 * n + 12 * n + 36 * nv + 4 * n + ((48 + 12 * c) * n if grads_cleared else 4 * n),
        "DepthSort": 80 * nv,
        "PrefixSumGaussHits": 12 * nv,
        "ProjectVisible": (84 + 12 * c) * nv,   # separate launch only for frames without intersections
        # K5 also gathers the records into depth order (the former K4) and clears the backward's v_combined
        "MapGaussiansToIntersect": 4 * nv + 76 * nv_l + 8 * ni_l + 40 * nv,
        # high-digit pass (hist 4 + scatter 8 + 8) + the bucket kernel that finishes the order and writes the offsets table
        # (8 + 8 per pair, 8 per tile); GetTileOffsets only exists as a launch of its own on the LSD path (BH_TILE_SORT_LSD, > 16 M pairs)
        "TileSort": 36 * ni_l + 8 * tiles,
        "GetTileOffsets": 4 * ni_l + 8 * tiles,
        "Rasterize": 44 * ni_blended + 16 * pixels,
        # pass A: image + GT in, the nine SSIM-partial planes out; pass B: image + GT + the planes in (once: the halo re-read is
        # not algorithmic), dL/dimg out  (loss_fused.hip)
        "ImageLoss": (16 + 4 + 36) * pixels,
        "ImageLossBackward": (16 + 4 + 36 + 16) * pixels,
        "RasterizeBackwards": 80 * ni_blended + 32 * pixels,
        "ProjectBackwards": (88 + 12 * c) * nv + (48 + 12 * c) * nv,
        "OptimizerStep": 28 * 11 * n + (20 * 3 * c + 8) * n + 36 * n,  # Adam x3 + refine statistics + noise, one launch
    }


DUMP_BUDGET = 64 * 10**6   # bytes of --dump-outputs in all (64 MB), .npy headers included


def dump_outputs(out_dir, arrays, n):
    """arrays (name -> float32 / float64 host array) -> out_dir/<name>.npy.  Arrays with one row per splat are cut, when together
    they would not fit the budget, to the same seeded sample of rows (a function of n and the row size alone: the same rows in
    every run with the same arguments), whose indices go to sample_rows.npy."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    rows = {k: a for k, a in arrays.items() if a.ndim >= 1 and a.shape[0] == n and n > 1}
    fixed = {k: a for k, a in arrays.items() if k not in rows}
    room = DUMP_BUDGET - 256 * (len(arrays) + 1) - sum(a.nbytes for a in fixed.values())
    row_bytes = sum(a.nbytes // n for a in rows.values())
    out = dict(fixed)
    if rows and row_bytes * n > room:
        k = max(1, room // (row_bytes + 8))   # (+ 8: the row's index in sample_rows)
        idx = np.sort(np.random.default_rng(0xD0A7).choice(n, size=min(n, k), replace=False))
        out.update({name: np.ascontiguousarray(a[idx]) for name, a in rows.items()})
        out["sample_rows"] = idx.astype(np.float64)
    else:
        out.update(rows)
    for name, a in out.items():
        assert a.dtype in (np.float32, np.float64), (name, a.dtype)
        np.save(os.path.join(out_dir, name + ".npy"), a)


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def spawn_ranks(args, argv):
    """`python bench.py --gpus N` without a launcher: re-execute through torch.distributed.run with N ranks."""
    dry = os.environ.get("BH_BENCH_DRYRUN") == "1"
    if not dry:
        import torch
        have = torch.cuda.device_count() if torch.cuda.is_available() else 0
        if have < args.gpus:
            raise SystemExit("bench.py --gpus %d: only %d GPU(s) visible on this node — refusing to print a line for fewer ranks than requested"
                             % (args.gpus, have))
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus), "--master-addr", "127.0.0.1",
           "--master-port", str(free_port()), os.path.abspath(__file__)] + argv
    return subprocess.call(cmd, env=env)


def dry_run(args):
    """BH_BENCH_DRYRUN=1 (tests/test_bench_spawn.py, CPU): every rank joins a gloo group and rank 0 prints the line's
    skeleton — checks the spawn / rendezvous / one-line contract without a GPU."""
    import torch
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    dist.init_process_group(backend="gloo")
    t = torch.ones(1)
    dist.all_reduce(t)
    if dist.get_rank() == 0:
        print(json.dumps({"metric": "dry run", "n_gpus": dist.get_world_size(), "ranks_joined": int(t.item()), "steps": args.steps,
                          "warmup": args.warmup, "full": args.full, "dry_run": True}), flush=True)
    dist.destroy_process_group()


def exchange_selfcheck(ba, synth, torch, ctx, dev, pg, rank, world, native, args):
    """Before anything is timed with N > 1 ranks: prove the exchange path that is about to be timed.
      (1) all-reduce of ones through each available path (the library's RCCL communicator, the torch.distributed hook) == world;
      (1b) all-reduce of a 56 MB rank-weighted integer pattern == its closed form, bit for bit;
      (2) two train steps of a small scene from identical replicas through each path: parameters bit-identical across the
          ranks, and equal between the two paths to 1e-6 (beyond that only where Adam turned a gradient that is summation-
          order noise into a +-lr step: a bounded fraction; the fraction is recorded).
    Returns (use_native, record).  A failing native path falls back to the hook LOUDLY; if the hook fails too the run is
    refused (non-zero exit, no JSON line).  A 60-s watchdog refuses a hung collective the same way."""
    import threading
    import torch.distributed as dist
    t_start = time.perf_counter()
    done = threading.Event()

    def watchdog():
        if not done.wait(60.0):
            sys.stderr.write("bench.py: exchange self-check did not finish within 60 s (hung collective?) - refusing to time this run\n")
            sys.stderr.flush()
            os._exit(3)
    threading.Thread(target=watchdog, daemon=True).start()
    tile_mode = args.parallel == "tiles" and world > 1
    n, w, h = 20000, 256, 256
    scene = synth.make_scene(n, 0x5C, sh_degree=0, log_scale_range=(math.log(0.02), math.log(0.2)))
    cp = synth.default_camera_params(w, h)
    yaw = 0.0 if tile_mode else 0.03 * rank
    cam = ba.Camera(position=cp["pos"], rotation=(0.0, math.sin(yaw / 2.0), 0.0, math.cos(yaw / 2.0)), fov_x=cp["fov_x"], fov_y=cp["fov_y"], center_uv=cp["center_uv"])
    gt = torch.from_numpy(synth.synthetic_gt_packed(w, h, seed=11 + (0 if tile_mode else rank)).view("int32")).to(dev)
    batch = ba.SceneBatch(gt, cam.uniforms((w, h)))

    def run_path(use_native):
        ones = torch.ones(4096, device=dev)
        if use_native:
            # every RCCL entry point the library binds (all-reduce SUM / MAX, all-gather, grouped send / recv), checked inside the library
            ctx.comm_selftest()
            ctx.allreduce_sum(ones)
        else:
            dist.all_reduce(ones)
        torch.cuda.synchronize(dev)
        if not bool((ones == float(world)).all()):
            raise RuntimeError("all-reduce of ones gave %r ... expected %d everywhere" % (ones[:2].tolist(), world))
        # ... and of a rank-dependent pattern the size of the real gradient block (56 MB): sum_r (r+1) * (i mod 4096) is exact in f32
        big = (torch.arange(14 * 1024 * 1024, device=dev, dtype=torch.int32) % 4096).to(torch.float32)
        want = big * float(world * (world + 1) // 2)
        mine = big * float(rank + 1)
        if use_native:
            ctx.allreduce_sum(mine)
        else:
            dist.all_reduce(mine)
        torch.cuda.synchronize(dev)
        if not torch.equal(mine, want):
            raise RuntimeError("all-reduce of a 56 MB rank-weighted pattern is wrong in %d places" % int((mine != want).sum().item()))
        del big, want, mine
        splats = ba.Splats(scene["transforms"].copy(), scene["sh"].copy(), scene["raw_opac"].copy(), device=dev)
        tr = ba.SplatTrainer(ba.TrainConfig(exact_lists=args.lists == "exact"), median_scene_scale=3.0, process_group=None if use_native else pg, ctx=ctx,
                             partition=args.parallel, native_comm=use_native, sparse_exchange=args.exchange == "sparse", seed=0xB5EED)
        for _ in range(2):
            tr.step(batch, splats)
        torch.cuda.synchronize(dev)
        flat = torch.cat([splats.transforms.reshape(-1), splats.sh_coeffs.reshape(-1), splats.raw_opacities.reshape(-1)])
        if not bool(torch.isfinite(flat).all()):
            raise RuntimeError("non-finite parameters after two steps")
        ref = flat.clone()
        dist.broadcast(ref, src=0)
        same = torch.tensor([1 if torch.equal(ref, flat) else 0], device=dev)
        dist.all_reduce(same, op=dist.ReduceOp.MIN)
        if int(same.item()) != 1:
            raise RuntimeError("replicas are not bit-identical after two steps")
        return flat

    rec = {"world": world, "scene": "%d splats, %dx%d, 2 steps per path" % (n, w, h)}
    results = {}
    for name, use_native in (("native", True), ("torch", False)):
        if use_native and not native:
            rec[name] = "not available"
            continue
        try:
            results[name] = run_path(use_native)
            rec[name] = "ok"
        except Exception as e:   # every rank must reach the same verdict: a failure anywhere fails the path everywhere
            rec[name] = "FAILED: %s" % (e,)
        bad = torch.tensor([0 if rec[name] == "ok" else 1], device=dev)
        dist.all_reduce(bad, op=dist.ReduceOp.MAX)
        if int(bad.item()) and rec[name] == "ok":
            rec[name] = "FAILED on another rank"
            results.pop(name, None)
    if "native" in results and "torch" in results:
        d = (results["native"] - results["torch"]).abs()
        rec["paths_max_abs_diff"] = float(d.max().item())
        rec["paths_frac_beyond_1e-6"] = float((d > 1e-6).float().mean().item())
        # (two runs of the SAME path already differ in ~0.1 % of the entries: the backward's float atomics order its sums differently
        #  every launch and Adam turns a noise gradient's sign into a +-lr step; a wrong sum moves every visible splat)
        if rec["paths_frac_beyond_1e-6"] > 2e-2:
            rec["native"] = "FAILED: disagrees with the torch.distributed path (%.3g of the parameters beyond 1e-6, max %.3g)" % (rec["paths_frac_beyond_1e-6"], rec["paths_max_abs_diff"])
    use_native = native and rec.get("native") == "ok"
    if native and not use_native:
        sys.stderr.write("bench.py: the library communicator FAILED its self-check (%s) - timing the torch.distributed hook instead\n" % rec.get("native"))
    if not use_native and rec.get("torch") != "ok":
        sys.stderr.write("bench.py: no exchange path passed its self-check (%r) - refusing to time this run\n" % (rec,))
        sys.stderr.flush()
        os._exit(4)
    rec["timed_path"] = "native" if use_native else "torch"
    rec["seconds"] = round(time.perf_counter() - t_start, 2)
    done.set()
    return use_native, rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)   # 0.12 s of GPU time; 20 steps read 3-5 % slower (clock ramp)
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="after the timed steps, write what the headline's last timed step left to its caller (the updated splats, the "
                         "step's loss and counts) as DIR/<name>.npy, float32 / float64, at most 64 MB (a seeded sample of splat rows "
                         "beyond that, their indices in sample_rows.npy): two builds run with the same arguments compare output for output")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--sh-degree", type=int, default=0)
    ap.add_argument("--workload", default="1m_1080p")
    ap.add_argument("--splats", type=int, default=0, help="override the splat count (debug)")
    ap.add_argument("--full", action="store_true",
                    help="besides the headline, measure everything else: the per-stage table, rooflines and counters (rocprofv3 child runs), "
                         "the CPU baseline, the side measurements (training loop, other view counts, SH 3, non-saturating and object-centric "
                         "scenes, forward-only render; N > 1: exchange stages and A/B).  The --no-* options below leave parts of it out")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baseline")
    ap.add_argument("--no-extra", action="store_true", help="--full: skip the side measurements")
    ap.add_argument("--no-pmc", action="store_true", help="--full: do not re-run a short bench under rocprofv3 for the kernel trace and the counter figures (use the committed CSVs, marked stale)")
    ap.add_argument("--no-stages", action="store_true", help="--full: skip the per-stage HIP-event pass (child runs under rocprofv3 use it)")
    ap.add_argument("--views", type=int, default=2,
                    help="views each rank cycles through in the timed region (step k trains view k %% V).  2 (the default) is the reference's own "
                         "training bench: two cameras 2 units apart in x, alternating (crates/brush-bench-test/src/benches.rs:198-220); "
                         "1 = one camera replayed (the round 1-3 headline); >= 3 = an orbit of V cameras")
    ap.add_argument("--no-view-ids", action="store_true", help="do not tell the library which view a batch is (BhTrainBatch.view_id = 0): all views share one per-tile cut table (A/B)")
    ap.add_argument("--windows", type=int, default=3,
                    help="timed windows of --steps steps each (barrier + synchronize on both sides of every window); the line reports the MEDIAN "
                         "window as ms_per_step / value and all of them in `windows_ms_per_step`")
    ap.add_argument("--no-noise", action="store_true", help="leave out the two stochastic terms of the reference's default step (mean noise, background jitter)")
    ap.add_argument("--comm", choices=["torch", "native"], default="native",
                    help="N>1 gradient exchange: 'native' = the library's own RCCL communicator (bh_comm_init / built-in exchange in "
                         "bh_train_step, no Python callback per step; the unique id is broadcast over the torch process group); "
                         "'torch' = torch.distributed all_reduce (backend nccl = RCCL) from the exchange hook")
    ap.add_argument("--exchange", choices=["sparse", "dense"], default="sparse",
                    help="N>1 (cameras and tiles): 'sparse' = mask-keyed exchange (visible flags, then only the gradient rows of splats some rank "
                         "saw; dense fallback above half of the scene), 'dense' = one all-reduce of the whole exchange buffer")
    ap.add_argument("--allreduce", choices=["ring", "direct"], default="ring",
                    help="N>1: how long messages of the gradient exchange are summed: 'ring' = ncclAllReduce / all_reduce, 'direct' = reduce-scatter + "
                         "all-gather over grouped send / recv (every pair of GPUs of the node has its own xGMI link)")
    ap.add_argument("--feed", choices=["resident", "loader"], default="resident",
                    help="'resident' (the headline): the GT batch is already in HBM when the timed region starts; 'loader': every step "
                         "takes a fresh 1080p RGB8 host image through SceneLoader/BatchUploader (pinned ring + copy stream + device "
                         "packing) - the PCIe-inclusive rate quoted in DESIGN.md, never `value` of the headline line")
    ap.add_argument("--lists", choices=["sliced", "exact"], default="sliced",
                    help="'sliced' (bh_train_step's default): per-tile lists built in two depth slices, the far one only into tiles the near one "
                         "left unsaturated (same image / gradients); 'exact': every (tile, splat) pair listed and sorted, as the reference does")
    ap.add_argument("--near-share", type=float, default=0.0, help="--lists sliced: fix the near slice's share of the pair list (developer A/B; 0 = automatic)")
    ap.add_argument("--loop-steps", type=int, default=3000, help="steps of each mode of the `train_loop` sub-measurement (0 = skip it)")
    ap.add_argument("--loop-segment", type=int, default=500, help="steps per reported segment of `train_loop`")
    ap.add_argument("--loop-only", default="", help="run ONLY `train_loop`, for these comma-separated modes (cuts_view_ids, cuts_no_ids, exact_lists), and print its object as "
                                                    "the JSON line — what scripts/late_phase_stats.sh profiles under rocprofv3 (not the contract's line)")
    ap.add_argument("--loop-views", type=int, default=64, help="views of the `train_loop` sub-measurement's orbit")
    ap.add_argument("--parallel", choices=["cameras", "tiles"], default="cameras",
                    help="N>1: 'cameras' = data parallel, one view per rank (weak scaling, the headline); "
                         "'tiles' = ONE view partitioned by strips of tile rows (strong scaling, BASELINE.json configs[4])")
    args = ap.parse_args()

    if args.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    if args.steps < 1 or args.warmup < 0:
        raise SystemExit("--steps must be >= 1 and --warmup >= 0")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(spawn_ranks(args, sys.argv[1:]))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus and not (args.gpus == 1 and os.environ.get("BH_FORCE_PG") == "1"):
        raise SystemExit("bench.py: --gpus %d but the launcher started WORLD_SIZE=%d ranks" % (args.gpus, world))
    if os.environ.get("BH_BENCH_DRYRUN") == "1":
        return dry_run(args)

    import numpy as np
    import torch

    # the contract is ONE JSON line on stdout: keep the real stdout aside and point fd 1 at stderr, so that banners
    # printed by native libraries (RCCL prints its version to stdout when a communicator is created) cannot join it
    sys.stdout.flush()
    real_stdout = os.dup(1)
    os.dup2(2, 1)
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the hot path has no CPU fallback")
    if torch.cuda.device_count() <= local_rank:
        raise SystemExit("bench.py: rank %d has no device (only %d visible)" % (local_rank, torch.cuda.device_count()))
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    pg = None
    # BH_FORCE_PG=1: build the RCCL process group even for one rank (developer smoke test of the exchange path on a 1-GPU box)
    if world > 1 or os.environ.get("BH_FORCE_PG") == "1":
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29517")
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
        dist.init_process_group(backend="nccl", device_id=dev)  # nccl == RCCL on ROCm
        pg = dist.group.WORLD

    import ctypes
    import brush_amd as ba
    from brush_amd import synth, _ffi as _ffi_mod

    tile_mode = args.parallel == "tiles" and world > 1
    ctx = ba.get_context(dev)
    if args.near_share > 0:
        ba.set_list_slicing(args.near_share, ctx)
    native = args.comm == "native" and pg is not None   # (tiles: the library also exchanges the strips' halos itself)
    if native:
        import threading
        import torch.distributed as dist
        # rank 0's RCCL unique id travels over the process group that exists anyway (used for the barriers and the timing MAX)
        ids = [bytes(ba.Context.comm_unique_id()) if rank == 0 else None]
        dist.broadcast_object_list(ids, src=0, device=dev)
        # ncclCommInitRank blocks until every rank has joined: run it beside a timer, so that a rendezvous that never completes
        # (this communicator has never met more than one rank on hardware) costs 45 s and the native path, not the run
        init_result = {}

        def _init():
            try:
                ctx.comm_init(rank, world, ids[0])
                init_result["ok"] = True
            except Exception as e:  # both paths are RCCL; say which one ran (the line's "exchange.comm")
                init_result["err"] = e
        th = threading.Thread(target=_init, daemon=True)
        th.start()
        th.join(45.0)
        if not init_result.get("ok"):
            why = init_result.get("err", "no answer from ncclCommInitRank within 45 s")
            print("bench.py: library communicator unavailable (%s); using the torch.distributed exchange hook" % (why,), file=sys.stderr)
            native = False
        ok = torch.tensor([1 if native else 0], device=dev)
        dist.all_reduce(ok, op=dist.ReduceOp.MIN)
        if native and int(ok.item()) == 0:
            print("bench.py: another rank could not create its library communicator; every rank uses the torch.distributed exchange hook", file=sys.stderr)
            native = False
    selfcheck = None
    if pg is not None:
        native, selfcheck = exchange_selfcheck(ba, synth, torch, ctx, dev, pg, rank, world, native, args)

    def barrier():
        if pg is not None:
            import torch.distributed as dist
            dist.barrier()
        torch.cuda.synchronize(dev)

    def view_cameras(cp, nviews):
        """The cameras one rank cycles through.  V = 2: the reference's training bench (benches.rs:198-220: camera positions
        (0,0,z) and (2,0,z), identity rotation, batches[step % 2]) on the named config's camera; V >= 3: V cameras on a circle of
        radius 1 around the named camera's position, each yawed to keep looking at the scene's centre line.  Rank r adds a small yaw
        so that the ranks' gradients differ (data parallel over cameras); one frame split over the ranks uses the same camera."""
        base = 0.0 if tile_mode else 0.02 * rank
        cams = []
        for v in range(nviews):
            if nviews <= 2:
                pos, yaw = (cp["pos"][0] + 2.0 * v, cp["pos"][1], cp["pos"][2]), base
            else:
                ang = 2.0 * math.pi * v / nviews
                pos = (cp["pos"][0] + math.cos(ang) - 1.0, cp["pos"][1] + 0.5 * math.sin(ang), cp["pos"][2])
                yaw = base - math.atan2(pos[0] - cp["pos"][0], 7.0)   # towards the scene's centre line at mid depth
            rot = (0.0, math.sin(yaw / 2.0), 0.0, math.cos(yaw / 2.0))
            cams.append(ba.Camera(position=pos, rotation=rot, fov_x=cp["fov_x"], fov_y=cp["fov_y"], center_uv=cp["center_uv"]))
        return cams

    direct_checked = [False]

    def measure(workload, steps, warmup, with_stages, sh_degree=None, nviews=None, windows=1, exchange=None, algo=None, growth_stop_iter=None,
                capture=False):
        """Time `windows` windows of `steps` train steps of `workload`, cycling through `nviews` views; returns a dict of raw
        measurements (rank-local; dt = the median window).  exchange / algo: override --exchange / --allreduce (the N > 1 A/B);
        growth_stop_iter: TrainConfig.growth_stop_iter (1 = every step runs the blend backward without the refine weight);
        capture: also return, as host arrays, what the last timed step left to its caller (`outputs`, see --dump-outputs).
        Without --full it returns after the timed windows: no stage table, per-view counts, plain-replica time or forward-only render."""
        sh_degree = args.sh_degree if sh_degree is None else sh_degree
        exchange = exchange or args.exchange
        algo = algo or args.allreduce
        if native:
            ctx.set_option("grad_allreduce", algo)
            if algo == "direct" and world > 1 and not direct_checked[0]:
                ctx.comm_selftest()   # (with the option set it also checks the direct all-reduce against ncclAllReduce's sum: collective, once)
                direct_checked[0] = True
        nviews = max(1, args.views if nviews is None else nviews)
        scene, w, h = synth.config_scene(workload, sh_degree, n=args.splats or None)
        n = scene["transforms"].shape[0]
        coeffs = scene["sh"].shape[1]
        cp = synth.default_camera_params(w, h)
        cams = view_cameras(cp, nviews)
        cam = cams[0]   # rank 0's first view is the named config's camera
        splats = ba.Splats(scene["transforms"], scene["sh"], scene["raw_opac"], device=dev)
        batches = []
        for v, c in enumerate(cams):
            gt = torch.from_numpy(synth.synthetic_gt_packed(w, h, seed=7 + 100 * v + (0 if tile_mode else rank)).view(np.int32)).to(dev)
            # view ids: what a loader knows anyway (the view's index in the dataset + 1) — keys the per-tile depth cuts of the forward
            batches.append(ba.SceneBatch(gt, c.uniforms((w, h)), view_id=(0 if args.no_view_ids else v + 1)))
        batch = batches[0]
        # seed: the reference's default step draws the mean noise and jitters the background every step
        tcfg = ba.TrainConfig(exact_lists=args.lists == "exact")
        if growth_stop_iter is not None:
            tcfg.growth_stop_iter = int(growth_stop_iter)
        trainer = ba.SplatTrainer(tcfg, median_scene_scale=5.0, process_group=None if native else pg, ctx=ctx, partition=args.parallel,
                                  native_comm=native, sparse_exchange=exchange == "sparse", seed=None if args.no_noise else 0xB5EED, allreduce=algo)
        loader = None
        if args.feed == "loader":
            # the SAME views and ground-truth images as the resident feed (so that the two rates differ by the feed alone), as decoded
            # host RGB8 arrays: every step uploads one through the pinned ring, the copy stream and the device packing kernel
            host_views = []
            for v, c in enumerate(cams):
                packed = synth.synthetic_gt_packed(w, h, seed=7 + 100 * v + (0 if tile_mode else rank))
                rgb = np.stack([(packed >> np.uint32(8 * k)) & np.uint32(255) for k in range(3)], axis=-1).astype(np.uint8)
                host_views.append((np.ascontiguousarray(rgb), c.uniforms((w, h))))
            loader = ba.SceneLoader(host_views, seed=rank, slots=3, ctx=ctx)
        counter = [0]

        def next_batch():
            if loader is not None:
                return loader.next_batch()
            b = batches[counter[0] % nviews]   # benches.rs:214: batches[step % batches.len()]
            counter[0] += 1
            return b

        # Every timed window is a REPLICA of the same piece of the same training run (the scene trains while it is
        # timed, so windows taken one after the other are different workloads): parameters, Adam moments, RefineRecord, step counter
        # (= the noise / background streams), the view cycle and the library's per-view tables go back to their initial state, the
        # `warmup` untimed steps run, and steps [warmup, warmup + steps) are timed.  The windows' spread is then noise, not drift.
        init = (splats.transforms.clone(), splats.sh_coeffs.clone(), splats.raw_opacities.clone())

        def start_replica():
            splats.transforms.copy_(init[0])
            splats.sh_coeffs.copy_(init[1])
            splats.raw_opacities.copy_(init[2])
            trainer.state = None          # (re-created zeroed by the next step)
            trainer.step_count = 0
            counter[0] = 0
            ctx.check(ctx.lib.bh_forget_views(ctx._h))
            ctx.profile(0)
            for _ in range(warmup):
                trainer.step(next_batch(), splats)
            barrier()

        def view_stats():
            """per view: the counts, and how much of the per-tile lists the blend kernels actually consume before every pixel
            saturates (the forward shrinks each tile's list end to its last useful splat).  Exact-list renders: no table is touched."""
            out = []
            for c in cams:
                _, aux = ba.render_splats(splats, c, (w, h), (0.0, 0.0, 0.0), ba.RasterPass.Backward, ctx=ctx)
                to = aux.tile_offsets.to(torch.int64)
                out.append({"num_visible": aux.num_visible, "num_intersections": aux.num_intersections,
                            "intersections_blended": int((to[:, 1] - to[:, 0]).clamp(min=0).sum().item())})
                del aux, to
            return out

        # (the interpreter's cyclic collector stays out of the timed regions: a generation-2 sweep of this process' heap is a
        #  30-50 ms host stall that lands on whichever call happens to cross its allocation threshold)
        sliced = args.lists == "sliced"
        far0 = int(ctx.lib.bh_far_slices_queued(ctx._h))
        shares = []
        window_dt = []
        dominant = {}
        far_queued = 0
        for _ in range(max(1, windows)):
            start_replica()
            # timed region: HIP events only around the dominant kernel (2 per step); bracketing all ~15 stages
            # costs ~0.1 ms of host time per step, so the per-stage table comes from a separate untimed replica
            ctx.profile(2)
            ctx.profile_fetch()
            far0 = int(ctx.lib.bh_far_slices_queued(ctx._h))
            gc.collect()
            gc.disable()
            t0 = time.perf_counter()
            for _ in range(steps):
                trainer.step(next_batch(), splats)
                if sliced:
                    shares.append(float(ctx.lib.bh_last_list_share(ctx._h)))   # a host field: no synchronisation
            barrier()
            window_dt.append(time.perf_counter() - t0)
            gc.enable()
            far_queued += int(ctx.lib.bh_far_slices_queued(ctx._h)) - far0
            for k, (ms, calls) in ctx.profile_fetch().items():   # the dominant kernel over the timed steps of every window
                a = dominant.get(k, (0.0, 0))
                dominant[k] = (a[0] + ms, a[1] + calls)
        outputs = None
        if capture:   # the last window's last step: the splats updated in place, and the step's own figures
            last = trainer.stats()
            outputs = {"transforms": splats.transforms, "sh_coeffs": splats.sh_coeffs, "raw_opacities": splats.raw_opacities}
            outputs = {k: v.detach().to(device="cpu", dtype=torch.float32).numpy() for k, v in outputs.items()}
            outputs.update({"loss": np.array([last.loss], np.float64), "num_visible": np.array([last.num_visible], np.float64),
                            "num_intersections": np.array([last.num_intersections], np.float64)})
        if pg is not None:   # every window: the slowest rank's time
            import torch.distributed as dist
            tmax = torch.tensor(window_dt, dtype=torch.float64, device=dev)
            dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
            window_dt = [float(x) for x in tmax.tolist()]
        dt = sorted(window_dt)[len(window_dt) // 2]
        res = dict(scene=scene, cp=cp, w=w, h=h, n=n, coeffs=coeffs, dt=dt, window_dt=window_dt, nviews=nviews, loader=loader is not None,
                   list_share=(sum(shares) / len(shares)) if shares else 1.0, near_share_min=min(shares) if shares else 1.0,
                   near_share_max=max(shares) if shares else 1.0, far_slices_queued=far_queued, timed_steps=steps * max(1, windows), outputs=outputs)
        if not args.full:
            # a plain run: the headline needs nothing beyond the timed windows (the stats of their last step feed the N > 1 exchange record)
            res["stats"] = trainer.stats()
            ctx.profile(0)
            if loader is not None:
                loader.close()
            if native:
                ctx.set_option("grad_allreduce", args.allreduce)
            return res
        # one more replica of the timed steps WITHOUT the two HIP events on the dominant kernel (each is a barrier packet: ~6 us of
        # bubble in front of / behind that kernel): what a caller of bh_train_step gets; reported beside the contractual figure
        dt_plain = None
        if windows > 1:
            start_replica()
            gc.collect()
            gc.disable()
            t0 = time.perf_counter()
            for _ in range(steps):
                trainer.step(next_batch(), splats)
            barrier()
            dt_plain = time.perf_counter() - t0
            gc.enable()
        # one more replica, untimed: what the timed steps looked like at their first and last step (the work per frame moves while
        # the scene trains: the roofline's "bytes per launch" are the mean of the two), and — HIP events around every stage — the
        # per-stage table of exactly the timed steps
        start_replica()
        pv0 = view_stats()
        stages = {}
        if with_stages and not args.no_stages:
            ctx.profile(1)
            ctx.profile_fetch()
        for _ in range(steps):
            trainer.step(next_batch(), splats)
        barrier()
        if with_stages and not args.no_stages:
            # per STEP, not per call: a sliced forward that needs a second attempt enters some scopes twice
            stages = {k: (ms, steps) for k, (ms, calls) in ctx.profile_fetch().items()}
        ctx.profile(0)
        pv1 = view_stats()
        stages.update(dominant)   # the dominant kernel's duration is the one measured inside the timed windows
        st = trainer.stats()
        per_view = [{k: int(round((a[k] + b[k]) / 2.0)) for k in a} for a, b in zip(pv0, pv1)]
        for v, a, b in zip(per_view, pv0, pv1):
            v["intersections_blended_first_last_timed_step"] = [a["intersections_blended"], b["intersections_blended"]]
        isect_blended = int(round(sum(v["intersections_blended"] for v in per_view) / len(per_view)))
        nv_mean = int(round(sum(v["num_visible"] for v in per_view) / len(per_view)))
        ni_mean = int(round(sum(v["num_intersections"] for v in per_view) / len(per_view)))
        if loader is not None:
            loader.close()
        if native:
            ctx.set_option("grad_allreduce", args.allreduce)
        fwd_only = None
        if with_stages == "forward_only":
            # RasterPass::Forward (BASELINE.json configs[1]; crates/brush-bench-test/src/benches.rs:222-243): projection + sorts + lists +
            # blend into a packed rgba8 image, no visible[] / list shrinking / backward state; each call ends with the host having the
            # counts (the call's one readback), as the reference's render does.  Timed as wall time over back-to-back calls.
            fwd_only = {}
            far1 = int(ctx.lib.bh_far_slices_queued(ctx._h))
            for mode, sl in (("exact_lists", False), ("sliced_lists", True)):
                for _ in range(5):
                    ba.render_splats(splats, cam, (w, h), (0.0, 0.0, 0.0), ba.RasterPass.Forward, ctx=ctx, copy=False, sliced=sl)
                torch.cuda.synchronize(dev)
                reps = 50
                per_call = []
                gc.collect()
                gc.disable()
                t0 = time.perf_counter()
                for _ in range(reps):
                    tc = time.perf_counter()
                    ba.render_splats(splats, cam, (w, h), (0.0, 0.0, 0.0), ba.RasterPass.Forward, ctx=ctx, copy=False, sliced=sl)
                    per_call.append(time.perf_counter() - tc)
                torch.cuda.synchronize(dev)
                fwd_only[mode] = round((time.perf_counter() - t0) / reps * 1e3, 4)
                gc.enable()
                if os.environ.get("BH_BENCH_DEBUG"):
                    pc = sorted(per_call)
                    print("forward_only %s: per-call host ms min %.3f median %.3f max %.3f (call %d)" % (mode, pc[0] * 1e3, pc[len(pc) // 2] * 1e3, pc[-1] * 1e3, per_call.index(pc[-1])), file=sys.stderr)
                if sl:
                    fwd_only["near_share"] = round(float(ctx.lib.bh_last_list_share(ctx._h)), 4)
                    fwd_only["far_slices_queued"] = int(ctx.lib.bh_far_slices_queued(ctx._h)) - far1
        res.update(stages=stages, stats=st, isect_blended=isect_blended, nv=nv_mean, ni=ni_mean, per_view=per_view, forward_only=fwd_only, dt_plain=dt_plain)
        return res

    def blend_rooflines(m, steps):
        """HBM and VALU rooflines of the two blend kernels from one measurement."""
        nv, ni, ib = m["nv"], m["ni"], m["isect_blended"]
        pixels = m["w"] * m["h"]
        dom_ms = m["stages"].get("RasterizeBackwards", (0.0, 0))
        dom_ms = dom_ms[0] / max(dom_ms[1], 1)
        touched = 80 * ib + 32 * pixels
        listed = 80 * ni + 32 * pixels
        ach = touched / 1e9 / (dom_ms * 1e-3) if dom_ms > 0 else 0.0
        hbm = {"bound": "hbm", "bound_note": "reported because the contract asks for it: the kernel is VALU-issue bound, see roofline_valu", "kernel": "rasterize_backward_kernel", "achieved": round(ach, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
               "frac": round(ach / HBM_PEAK_GBS, 4), "bytes_per_launch": touched, "avg_launch_ms": round(dom_ms, 4),
               "avg_launch_ms_clock": "HIP events carried by the kernel's own dispatch packet (hipExtLaunchKernelGGL start / stop events on the ctx stream), every launch "
                                      "of the timed steps of every window, mean over them and over the views.  kernel_trace.kernels holds the same kernel's begin/end "
                                      "timestamps from a rocprofv3 child run of this command over the SAME steps (same warm-up, same step count, same initial state)",
               "intersections_listed": ni, "intersections_blended": ib,
               "frac_listed": round(listed / 1e9 / (dom_ms * 1e-3) / HBM_PEAK_GBS, 4) if dom_ms > 0 else 0.0,
               "note": "achieved = bytes the launch touches (80 B per BLENDED intersection + 32 B per pixel) / measured duration. frac_listed is the "
                       "SURVEY 8d figure that charges every LISTED intersection (80*I + 32*P): the kernel stops each tile once all its pixels "
                       "saturate, so that figure counts reads it never makes and can exceed 1. The kernel is VALU-issue bound: see roofline_valu. "
                       "`traffic` exceeds the algorithmic bytes by design since round 6: the backward works on 128-entry segments of the tiles' lists, each of "
                       "which reads a 4 KB pixel-state checkpoint and its tile's pixels (DESIGN.md 4, K17), and the XCD bands are dealt in chunks of four tiles, so a splat's "
                       "row is fetched into every L2 whose XCD blends one of its tiles (FETCH_SIZE counts L2 misses, Infinity-Cache hits included) - with whole tiles and "
                       "contiguous bands (options bwd_jobs=0, band_mode=0) the ratio is 0.97."}
        valu = {}
        for stage, kern in (("RasterizeBackwards", "rasterize_backward_kernel"), ("Rasterize", "rasterize_kernel")):
            ms, calls = m["stages"].get(stage, (0.0, 0))
            ms = ms / max(calls, 1)
            if ms <= 0:
                continue
            per, src = valu_per_isect(kern)
            insts = per * ib
            g = insts / 1e9 / (ms * 1e-3)
            valu[kern] = {"bound": "valu", "achieved": round(g, 1), "peak": VALU_PEAK_GINST, "unit": "G wave-instructions/s", "frac": round(g / VALU_PEAK_GINST, 4),
                          "valu_insts_per_blended_intersection": per, "source": src, "avg_launch_ms": round(ms, 4),
                          "ns_per_blended_intersection": round(ms * 1e6 / max(ib, 1), 3),
                          "G_pixel_splat_evals_per_s": round(256.0 * ib / 1e9 / (ms * 1e-3), 1)}
        return hbm, valu

    def train_loop(workload, nviews, total_steps, refine_every=200, segment=500, probe_steps=8, modes=("cuts_view_ids", "cuts_no_ids", "exact_lists")):
        """The reference's training LOOP at the named size (crates/brush-process/src/train_stream.rs:220-306: next_batch -> step ->
        refine every `refine_every` steps, brush-train/src/config.rs:59) on a scene that CONVERGES: a hidden TEACHER —
        the named workload's splats — is rendered by this library from `nviews` cameras on an orbit into RGB8 host images before
        anything is timed (a multi-view-consistent dataset, the scripts/train_synthetic.py recipe at 1 M splats / 1080p); the STUDENT
        starts as a perturbed copy (means, rotations, scales, colours and opacities off) and is trained with the default stochastic
        step through SceneLoader (a fresh host image per step: pinned ring, copy stream, device packing), refine on the device.
        Three runs from the same student: per-tile cuts keyed by the loader's view ids | keyed by the camera (BhTrainBatch.view_id = 0)
        | complete lists as the reference builds them.  Reported per `segment` steps: ms per step (wall, over the segment's steps
        before its probe), near share, second attempts, and — from the segment's last `probe_steps` steps, run with HIP events around
        every stage and a host sync per step, excluded from the segment's time — blended pairs per frame, K16 / K17 time and ns per
        blended pair; PSNR of the student on two HELD-OUT orbit cameras against the teacher; the splat count."""
        scene, w, h = synth.config_scene(workload, args.sh_degree)
        cp = synth.default_camera_params(w, h)
        cams = view_cameras(cp, nviews)
        teacher = ba.Splats(scene["transforms"], scene["sh"], scene["raw_opac"], device=dev)
        bg0 = (0.0, 0.0, 0.0)
        host_views = []
        for c in cams:   # "decoded dataset images": RGB8 host arrays of the teacher, rendered before the timed region
            img, _ = ba.render_splats(teacher, c, (w, h), bg0, ba.RasterPass.Backward, ctx=ctx)
            host_views.append((np.ascontiguousarray((img[..., :3].clamp(0.0, 1.0) * 255.0 + 0.5).to(torch.uint8).cpu().numpy()), c.uniforms((w, h))))
        # held-out views: orbit positions half a step between two training cameras
        held = []
        for k in (0, nviews // 2):
            ang = 2.0 * math.pi * (k + 0.5) / nviews
            pos = (cp["pos"][0] + math.cos(ang) - 1.0, cp["pos"][1] + 0.5 * math.sin(ang), cp["pos"][2])
            yaw = -math.atan2(pos[0] - cp["pos"][0], 7.0)
            hc = ba.Camera(position=pos, rotation=(0.0, math.sin(yaw / 2.0), 0.0, math.cos(yaw / 2.0)), fov_x=cp["fov_x"], fov_y=cp["fov_y"], center_uv=cp["center_uv"])
            ref, _ = ba.render_splats(teacher, hc, (w, h), bg0, ba.RasterPass.Backward, ctx=ctx)
            held.append((hc, ref[..., :3].clamp(0.0, 1.0).clone()))
        del teacher
        # the student: the teacher's splats, every parameter group off (seeded)
        rng = np.random.default_rng(0x57D)
        n0 = scene["transforms"].shape[0]
        st_tr = scene["transforms"].copy()
        st_tr[:, 0:3] += rng.normal(scale=0.02, size=(n0, 3)).astype(np.float32)
        st_tr[:, 3:7] += rng.normal(scale=0.15, size=(n0, 4)).astype(np.float32)
        st_tr[:, 7:10] += rng.normal(loc=-0.1, scale=0.25, size=(n0, 3)).astype(np.float32)
        st_sh = scene["sh"].copy()
        st_sh[:, 0, :] = 0.5 * st_sh[:, 0, :] + rng.normal(scale=0.3, size=(n0, 3)).astype(np.float32)
        st_op = (scene["raw_opac"] + rng.normal(scale=1.0, size=n0).astype(np.float32)).astype(np.float32)

        def held_out_psnr(spl):
            vals = []
            for hc, ref in held:
                img, _ = ba.render_splats(spl, hc, (w, h), bg0, ba.RasterPass.Backward, ctx=ctx)
                mse = float(((img[..., :3].clamp(0.0, 1.0) - ref) ** 2).mean().item())
                vals.append(99.0 if mse <= 0.0 else -10.0 * math.log10(mse))
            return round(sum(vals) / len(vals), 3)

        def frame_blended():
            ro = _ffi_mod.BhRenderOut()
            ctx.check(ctx.lib.bh_last_render_out(ctx._h, ctypes.byref(ro)))
            to = ba.host._view(ro.tile_offsets, (ro.num_tiles, 2), torch.int32, dev).to(torch.int64)
            return int((to[:, 1] - to[:, 0]).clamp(min=0).sum().item()), int(ro.num_intersections), int(ro.num_visible)

        out = {"workload": "%s: a hidden teacher (the workload's %d splats) rendered from %d orbit cameras into RGB8 host images; the student (a perturbed copy) is trained "
                           "through SceneLoader for %d steps with the default stochastic step, refine every %d steps" % (workload, n0, nviews, total_steps, refine_every),
               "reference": "crates/brush-process/src/train_stream.rs:220-306; refine_every: crates/brush-train/src/config.rs:59",
               "segment_steps": segment, "probe_steps_per_segment": probe_steps,
               "segments_are": "ms_per_step: wall time of the segment's steps before its probe (refine calls included); k16 / k17: HIP events around the blend kernels over "
                               "the segment's last %d steps (each followed by a host sync to count the frame's blended pairs; not in the segment's time); psnr: the student "
                               "on two held-out orbit cameras against the teacher" % probe_steps}
        for mode in modes:
            splats = ba.Splats(st_tr.copy(), st_sh.copy(), st_op.copy(), device=dev)
            cfg = ba.TrainConfig(exact_lists=mode == "exact_lists", refine_every=refine_every)
            trainer = ba.SplatTrainer(cfg, median_scene_scale=5.0, ctx=ctx, seed=0xB5EED)
            trainer.set_bounds(*ba.splat_bounds(splats, ctx=ctx))
            ctx.check(ctx.lib.bh_forget_views(ctx._h))
            psnr0 = held_out_psnr(splats)
            ctx.check(ctx.lib.bh_forget_views(ctx._h))
            loader = ba.SceneLoader(host_views, seed=3, slots=3, ctx=ctx)
            try:
                for _ in range(4):   # buffers, code objects
                    trainer.step(loader.next_batch(), splats)
                torch.cuda.synchronize(dev)
                far0 = far_seg = int(ctx.lib.bh_far_slices_queued(ctx._h))
                shares, n_over_time, refine_s = [], [[0, splats.num_splats()]], 0.0
                segments, seg_shares, seg_t, seg_steps, seg_refine_s = [], [], 0.0, 0, 0.0
                total_t = 0.0
                gc.collect()
                gc.disable()
                t0 = time.perf_counter()
                it = 0
                while it < total_steps:
                    seg_end = min(total_steps, (it // segment + 1) * segment)
                    seg_first = it + 1
                    probe_from = max(it, seg_end - probe_steps)
                    # ---- the segment's timed steps
                    while it < probe_from:
                        it += 1
                        b = loader.next_batch()
                        if mode == "cuts_no_ids":
                            b.view_id = 0
                        trainer.step(b, splats)
                        if mode != "exact_lists":
                            seg_shares.append(float(ctx.lib.bh_last_list_share(ctx._h)))
                        if it % refine_every == 0 and it < total_steps:
                            tr0 = time.perf_counter()
                            splats, _ = trainer.refine(it, splats)
                            seg_refine_s += time.perf_counter() - tr0
                            n_over_time.append([it, splats.num_splats()])
                        seg_steps += 1
                    torch.cuda.synchronize(dev)
                    seg_t = time.perf_counter() - t0
                    total_t += seg_t
                    far_now = int(ctx.lib.bh_far_slices_queued(ctx._h))
                    # ---- the probe: the segment's last steps, instrumented (not timed)
                    ctx.profile(1)
                    ctx.profile_fetch()
                    blended, listed_pairs, visible = [], [], []
                    while it < seg_end:
                        it += 1
                        b = loader.next_batch()
                        if mode == "cuts_no_ids":
                            b.view_id = 0
                        trainer.step(b, splats)
                        bl, ni_f, nv_f = frame_blended()
                        blended.append(bl); listed_pairs.append(ni_f); visible.append(nv_f)
                        if it % refine_every == 0 and it < total_steps:
                            splats, _ = trainer.refine(it, splats)
                            n_over_time.append([it, splats.num_splats()])
                    prof = ctx.profile_fetch()
                    ctx.profile(0)
                    psnr = held_out_psnr(splats)
                    mb = sum(blended) / max(1, len(blended))
                    k16 = prof.get("Rasterize", (0.0, 0))
                    k17 = prof.get("RasterizeBackwards", (0.0, 0))
                    k16_ms, k17_ms = k16[0] / max(1, len(blended)), k17[0] / max(1, len(blended))
                    seg = {"steps": [seg_first, seg_end], "timed_steps": seg_steps,
                           "ms_per_step": round(seg_t / max(1, seg_steps) * 1e3, 4),
                           "ms_per_step_without_refine_calls": round((seg_t - seg_refine_s) / max(1, seg_steps) * 1e3, 4),
                           "blended_pairs_per_frame": int(round(mb)), "pairs_per_frame": int(round(sum(listed_pairs) / max(1, len(listed_pairs)))),
                           "visible_per_frame": int(round(sum(visible) / max(1, len(visible)))),
                           "k16_ms": round(k16_ms, 4), "k17_ms": round(k17_ms, 4),
                           "k16_ns_per_blended_pair": round(k16_ms * 1e6 / max(mb, 1.0), 4), "k17_ns_per_blended_pair": round(k17_ms * 1e6 / max(mb, 1.0), 4),
                           "psnr_held_out": psnr, "splats": splats.num_splats(),
                           # every stage of the probe's steps (HIP events around the stage: multi-launch stages read a few us long)
                           "stages_us": {k: round(ms / max(1, len(blended)) * 1e3, 1) for k, (ms, c) in prof.items()}}
                    if mode != "exact_lists":
                        cut = [x for x in seg_shares if x < 1.0]
                        seg.update({"near_share_mean": round(sum(seg_shares) / max(1, len(seg_shares)), 4), "second_attempts": far_now - far_seg,
                                    "frames_with_complete_lists": len(seg_shares) - len(cut)})
                    segments.append(seg)
                    shares += seg_shares
                    refine_s += seg_refine_s
                    far_seg = int(ctx.lib.bh_far_slices_queued(ctx._h))
                    seg_shares, seg_steps, seg_refine_s = [], 0, 0.0
                    ctx.check(ctx.lib.bh_sync(ctx._h))
                    t0 = time.perf_counter()
                gc.enable()
                st = trainer.stats()
                timed = sum(sg["timed_steps"] for sg in segments)
                e = {"ms_per_step": round(total_t / max(1, timed) * 1e3, 4), "views_per_s": round(timed / max(total_t, 1e-12), 2),
                     "ms_per_step_without_refine_calls": round((total_t - refine_s) / max(1, timed) * 1e3, 4), "refine_calls": len(n_over_time) - 1,
                     "refine_ms_each": round(refine_s / max(1, len(n_over_time) - 1) * 1e3, 3),
                     "late_phase_ms_per_step": segments[-1]["ms_per_step"], "psnr_held_out": [psnr0, segments[-1]["psnr_held_out"]],
                     "segments": segments,
                     "splats_over_time": n_over_time, "last_step": {"num_visible": int(st.num_visible), "num_intersections": int(st.num_intersections), "loss": round(float(st.loss), 5)}}
                if shares:
                    cut = [x for x in shares if x < 1.0]
                    e.update({"second_attempts": int(ctx.lib.bh_far_slices_queued(ctx._h)) - far0,
                              "near_share": {"min": round(min(shares), 4), "mean": round(sum(shares) / len(shares), 4), "max": round(max(shares), 4)},
                              "frames_with_complete_lists": len(shares) - len(cut)})
                out[mode] = e
            finally:
                gc.enable()
                ctx.profile(0)
                loader.close()
            del splats, trainer
        if len(modes) < 3:
            return out
        best = min(("cuts_view_ids", "cuts_no_ids", "exact_lists"), key=lambda k: out[k]["ms_per_step"])
        out["fastest"] = best
        out["cuts_vs_exact"] = round(out["exact_lists"]["ms_per_step"] / out["cuts_view_ids"]["ms_per_step"], 4)
        out["cuts_vs_exact_late_phase"] = round(out["exact_lists"]["late_phase_ms_per_step"] / out["cuts_view_ids"]["late_phase_ms_per_step"], 4)
        out["no_ids_vs_ids"] = round(out["cuts_no_ids"]["ms_per_step"] / out["cuts_view_ids"]["ms_per_step"], 4)
        return out

    if args.loop_only:
        lo = train_loop(args.workload, max(2, args.loop_views), args.loop_steps, segment=max(50, args.loop_segment), modes=tuple(x for x in args.loop_only.split(",") if x))
        os.write(real_stdout, (json.dumps({"train_loop": lo}) + "\n").encode())
        return
    extras = args.full and not args.no_extra   # the side measurements
    m = measure(args.workload, args.steps, args.warmup, "forward_only" if (world == 1 and extras) else True, windows=args.windows,
                capture=bool(args.dump_outputs))
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, m["outputs"], m["n"])

    loop = None
    if world == 1 and extras and args.loop_steps > 0 and args.feed == "resident" and not args.splats and args.lists == "sliced":
        loop = train_loop(args.workload, max(2, args.loop_views), args.loop_steps, segment=max(50, args.loop_segment))

    # the round 1-3 headline (ONE camera replayed: the slicing feedback, the tile order and every cache see the same frame every
    # step) next to the multi-view number, and an 8-view orbit
    view_runs = None
    if world == 1 and extras and args.feed == "resident" and not args.splats:
        view_runs = {}
        for nvw in (1, 8):
            if nvw == args.views:
                continue
            vs = max(10, min(args.steps, 40))
            mv = measure(args.workload, vs, 2 * nvw, False, nviews=nvw, windows=1)
            view_runs["views_%d" % nvw] = {"views": nvw, "steps": vs, "ms_per_step": round(mv["dt"] / vs * 1e3, 4), "views_per_s": round(vs / mv["dt"], 2),
                                           "near_share_min": round(mv["near_share_min"], 4), "near_share_max": round(mv["near_share_max"], 4),
                                           "far_slices_queued": mv["far_slices_queued"],
                                           "num_intersections_per_view": [v["num_intersections"] for v in mv["per_view"]],
                                           "intersections_blended_per_view": [v["intersections_blended"] for v in mv["per_view"]]}

    extra = None
    if world == 1 and extras and args.workload == "1m_1080p" and args.feed == "resident" and not args.splats:
        ex_steps = max(10, min(args.steps, 30))
        me = measure("1m_1080p_lowopac", ex_steps, 3, True)
        ehbm, evalu = blend_rooflines(me, ex_steps)
        est = me["stats"]
        extra = {"workload": "1m_1080p_lowopac: the configs[2] scene with opacities U(0.02, 0.1) instead of U(0.05, 0.95) — tiles do not saturate early, "
                             "the blend kernels consume %.0f %% of every list (NOT a BASELINE.json config; context for the blend kernels only)"
                             % (100.0 * me["isect_blended"] / max(me["ni"], 1)),
                 "steps": ex_steps, "ms_per_step": round(me["dt"] / ex_steps * 1e3, 4), "views_per_s": round(ex_steps / me["dt"], 2),
                 "views": me["nviews"], "num_visible": me["nv"], "num_intersections": me["ni"], "intersections_blended": me["isect_blended"],
                 "list_share": me["list_share"], "far_slices_queued": me["far_slices_queued"],
                 "roofline": ehbm, "roofline_valu": evalu,
                 "stages_ms": {k: round(ms / max(c, 1), 4) for k, (ms, c) in me["stages"].items()}}

    centered = None
    if world == 1 and extras and args.workload == "1m_1080p" and args.feed == "resident" and not args.splats and args.sh_degree == 0:
        # an object in front of an empty background (what a NeRF-synthetic view looks like to the blend kernels: half of the tiles are
        # empty, the heaviest blends 15x the mean): the frame on which one wave per TILE made the backward last as long as its
        # heaviest tile.  With the backward's jobs (checkpointed 128-entry segments, the default) and, same call, with whole tiles.
        c_steps = max(10, min(args.steps, 30))
        mc = measure("1m_1080p_centered", c_steps, 3, True)
        ctx.set_option("bwd_jobs", 0)
        try:
            mc0 = measure("1m_1080p_centered", c_steps, 3, True)
        finally:
            ctx.set_option("bwd_jobs", 1)
        # ... and with every tile blended by ONE wave (no split tiles: the forward then lasts as long as its heaviest tile)
        ctx.set_option("k16_split", 0)
        try:
            mc1 = measure("1m_1080p_centered", c_steps, 3, True)
        finally:
            ctx.set_option("k16_split", 250)
        stg = lambda mm, k: round(mm["stages"].get(k, (0.0, 0))[0] / max(mm["stages"].get(k, (0.0, 1))[1], 1), 4)   # noqa: E731
        centered = {"workload": "1m_1080p_centered: the configs[2] splats squeezed into the central half of the frustum (NOT a BASELINE.json config; an object-centric frame: "
                                "%d intersections, %d blended)" % (mc["ni"], mc["isect_blended"]),
                    "steps": c_steps, "ms_per_step": round(mc["dt"] / c_steps * 1e3, 4), "k16_ms": stg(mc, "Rasterize"), "k17_ms": stg(mc, "RasterizeBackwards"),
                    "whole_tile_backward": {"option": "bwd_jobs=0", "ms_per_step": round(mc0["dt"] / c_steps * 1e3, 4), "k17_ms": stg(mc0, "RasterizeBackwards")},
                    "one_wave_per_tile_forward": {"option": "k16_split=0", "ms_per_step": round(mc1["dt"] / c_steps * 1e3, 4), "k16_ms": stg(mc1, "Rasterize")}}

    sh3 = None
    if world == 1 and extras and args.workload == "1m_1080p" and args.feed == "resident" and not args.splats and args.sh_degree == 0:
        s3_steps = max(10, min(args.steps, 30))
        m3 = measure("1m_1080p", s3_steps, 3, True, sh_degree=3)
        sh3 = {"workload": "1m_1080p at SH degree 3 (the reference's ModelConfig default, 16 coefficients per splat)", "steps": s3_steps,
               "ms_per_step": round(m3["dt"] / s3_steps * 1e3, 4), "views_per_s": round(s3_steps / m3["dt"], 2),
               "views": m3["nviews"], "num_visible": m3["nv"], "num_intersections": m3["ni"], "list_share": m3["list_share"], "far_slices_queued": m3["far_slices_queued"],
               "stages_ms": {k: round(ms / max(c, 1), 4) for k, (ms, c) in m3["stages"].items()}}

    per_rank = None
    if pg is not None:
        # what every rank put on the wire in its last step (an all-reduce moves ~2 (N-1)/N of its payload per rank): the first
        # SCALE record should be readable without a second run
        import torch.distributed as dist
        st_r = m["stats"]
        c3 = 3 * m["coeffs"]
        pad4 = lambda x: (x + 3) & ~3   # noqa: E731
        dense_bytes = 4 * (pad4(m["n"]) + pad4(10 * m["n"]) + pad4(c3 * m["n"]) + pad4(m["n"]) + (pad4(m["n"]) if tile_mode else 0))
        if args.exchange == "sparse" and st_r.exchange_rows > 0:
            payload = 4 * pad4(m["n"]) + 4 * st_r.exchange_rows * (11 + c3 + (1 if tile_mode else 0))
        else:
            payload = dense_bytes
        mine = {"rank": rank, "rows_last_step": int(st_r.exchange_rows), "allreduce_payload_bytes_last_step": int(payload),
                "dense_payload_bytes": int(dense_bytes), "num_visible": int(st_r.num_visible), "num_intersections": int(st_r.num_intersections),
                "ms_per_step_local": round(m["dt"] / args.steps * 1e3, 4), "far_slices_queued": m["far_slices_queued"]}
        per_rank = [None] * world
        dist.all_gather_object(per_rank, mine)

    late = None
    if world == 1 and extras and args.workload == "1m_1080p" and args.feed == "resident" and not args.splats and args.sh_degree == 0:
        # the second half of a default training run (iter >= growth_stop_iter = 15000 of 30000, config.rs:72): nobody reads the refine
        # weight any more (train.rs:589-614), bh_train_step runs the blend backward without it.  Same protocol as the headline.
        ml = measure(args.workload, args.steps, args.warmup, True, windows=1, growth_stop_iter=1)
        k17 = ml["stages"].get("RasterizeBackwards", (0.0, 0))
        late = {"what": "the headline's steps with TrainConfig.growth_stop_iter = 1: every step's blend backward runs without the refine weight "
                        "(what steps >= growth_stop_iter of a training run execute; crates/brush-train/src/train.rs:589-614, config.rs:72)",
                "ms_per_step": round(ml["dt"] / args.steps * 1e3, 4), "views_per_s": round(args.steps / ml["dt"], 2),
                "k17_ms_hip_events_around_the_stage": round(k17[0] / max(k17[1], 1), 4)}

    def full_figures(m, steps, ms_per_step):
        """--full: the per-stage table (kernel timestamps of a rocprofv3 child run, else HIP events), the rooflines and the counters."""
        n, w, h, coeffs = m["n"], m["w"], m["h"], m["coeffs"]
        nv, ni = m["nv"], m["ni"]   # means over the views of the timed region
        pixels, tiles = w * h, ((w + 15) // 16) * ((h + 15) // 16)
        sb = stage_bytes(n, nv, ni, m["isect_blended"], pixels, tiles, coeffs, list_share=m.get("list_share", 1.0),
                         grads_cleared=(world > 1 or bool(os.environ.get("BH_FORCE_PG")) or bool(os.environ.get("BH_TRAIN_ZERO_GRADS"))))
        # per-stage GPU time: the kernels' own timestamps (a child run under rocprofv3 --kernel-trace) when rocprofv3 is there,
        # else HIP events around each stage — which are host-bound while they record and read multi-launch stages too long
        headline_n1 = args.workload == "1m_1080p" and args.sh_degree == 0 and not args.splats and world == 1 and args.feed == "resident"
        ktrace = kernel_trace_inrun(args) if (headline_n1 and not args.no_pmc) else None
        stage_ms = {name: ms / max(calls, 1) for name, (ms, calls) in m["stages"].items() if calls}
        stage_src = "HIP events around each stage (host-bound while recording: multi-launch stages read long)"
        if ktrace:
            # ONE source for the whole table: the child's kernel timestamps over the same steps the parent timed.  The dominant kernel's
            # duration inside the PARENT's timed windows (its own dispatch events) stays what the rooflines are computed from.
            dom = stage_ms.get("RasterizeBackwards")
            stage_ms = {k: v / 1e3 for k, v in ktrace["stages_us"].items()}
            stage_src = ("kernel timestamps of the timed steps: rocprofv3 --kernel-trace over a child run of this command (same warm-up, the same %d steps, "
                         "same initial state)" % ktrace["steps"])
            for k, v in stage_ms.items():
                if k != "RasterizeBackwards":
                    m["stages"][k] = (v, 1)
            if dom:
                m["stages"]["RasterizeBackwards"] = (dom, 1)
        stage_out = {}
        for name, avg in stage_ms.items():
            if name == "ZeroGradBuffers" and avg < 0.004:
                continue   # an empty scope (the fills ride on K1 / K5): nothing to report
            e = {"ms": round(avg, 4)}
            if name in sb and avg > 0:
                e["MB"] = round(sb[name] / 1e6, 2)
                e["GBps"] = round(sb[name] / 1e9 / (avg * 1e-3), 1)
                if name in CACHE_RESIDENT:
                    e["cache_resident"] = CACHE_RESIDENT[name]
                else:
                    e["hbm_frac"] = round(e["GBps"] / HBM_PEAK_GBS, 4)
            stage_out[name] = e
        fwd_names = ["ProjectSplats", "DepthSort", "PrefixSumGaussHits", "ProjectVisible", "MapGaussiansToIntersect", "TileSort", "GetTileOffsets", "Rasterize"]
        bwd_names = ["ZeroGradBuffers", "RasterizeBackwards", "ProjectBackwards"]
        fwd_ms = sum(stage_out[k]["ms"] for k in fwd_names if k in stage_out)
        bwd_ms = sum(stage_out[k]["ms"] for k in bwd_names if k in stage_out)
        fwd_src = stage_src
        hbm, valu = blend_rooflines(m, steps)
        # the committed PMC passes were taken on the headline workload: no counter figure for any other
        headline = args.workload == "1m_1080p" and args.sh_degree == 0 and not args.splats and not tile_mode
        # counters: measured now, in child runs of this very command under rocprofv3 --pmc (one pass per counter group, as the guide
        # prescribes; never combined with tracing) — or, without rocprofv3 / with --no-pmc, the committed CSVs marked stale
        live = pmc_inrun(args) if (headline and world == 1 and not args.no_pmc) else None
        if live and live.get("rasterize_backward_kernel", {}).get("hbm_bytes") is not None:
            hbm["traffic"] = live["rasterize_backward_kernel"]["hbm_bytes"]
            hbm["traffic_source"] = "rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this run (FETCH x2: gfx950 correction, MI355X_MICROARCH.md)"
            hbm["traffic_stale"] = False
        else:
            traffic, traffic_src = pmc_traffic_bytes("rasterize_backward_kernel") if headline else (None, None)
            hbm["traffic"] = traffic
            hbm["traffic_source"] = traffic_src
            hbm["traffic_stale"] = traffic is not None
        if live:
            for kern, v in valu.items():
                per = live.get(kern, {}).get("valu_per_blended_isect")
                if per:
                    g = per * m["isect_blended"] / 1e9 / (v["avg_launch_ms"] * 1e-3)
                    v.update({"valu_insts_per_blended_intersection": round(per, 2), "source": "SQ_INSTS_VALU pass of this run", "stale": False,
                              "achieved": round(g, 1), "frac": round(g / VALU_PEAK_GINST, 4)})
        for v in valu.values():
            v.setdefault("stale", True)
        step_bytes = sum(sb[k] for k in stage_out if k in sb)
        return {
            "fwd_ms": round(fwd_ms, 4),
            "fwd_bwd_ms": round(fwd_ms + bwd_ms, 4),
            "fwd_bwd_source": fwd_src,
            "kernel_trace": ({"steps": ktrace["steps"], "kernels": ktrace["kernels"], "wall_us_per_step": ktrace.get("wall_us_per_step"),
                              "idle_us_per_step": ktrace.get("idle_us_per_step"),
                              "idle_is": "inside the SAME (child) run: from the first kernel's start to the last kernel's end of the timed steps, minus the kernels' "
                                         "own durations - the step's true idle time (kernel_ms_per_step vs ms_per_step compares two different runs, one of them "
                                         "under the profiler)"} if ktrace else None),
            "kernel_ms_per_step": round(sum(e["ms"] for e in stage_out.values()), 4),
            "roofline": hbm,
            "roofline_valu": valu,
            "step_hbm": {"bytes_per_step": step_bytes, "GBps": round(step_bytes / 1e9 / (ms_per_step * 1e-3), 1),
                         "frac": round(step_bytes / 1e9 / (ms_per_step * 1e-3) / HBM_PEAK_GBS, 4),
                         "note": "sum of the per-stage bytes (blend kernels: touched bytes) / ms_per_step"},
            "stages": stage_out,
        }

    final_out = None
    if rank == 0:
        steps = args.steps
        dt, st = m["dt"], m["stats"]
        n, w, h = m["n"], m["w"], m["h"]
        ms_per_step = dt / steps * 1e3
        out = {
            "metric": "train views/sec @ 1M Gaussians, 1080p (fwd + L1/SSIM loss + bwd + Adam per view)",
            "value": round((1 if tile_mode else world) * steps / dt, 3),
            "unit": "views/s",
            "n_gpus": world,
            "steps": steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 4),
            "higher_is_better": True,
            "scaling": "strong" if tile_mode else "weak",
            "vs_baseline": None,
            "dtype": "f32",
            "data": "synthetic" if not m["loader"] else "synthetic, a fresh host RGB8 image uploaded per step (PCIe-inclusive; not the headline)",
            "windows_ms_per_step": [round(x / steps * 1e3, 4) for x in m["window_dt"]],
            "windows_spread": round((max(m["window_dt"]) - min(m["window_dt"])) / max(dt, 1e-12), 4),
            "windows_are": "replicas: every window times steps [warmup, warmup + steps) of the same training run from the same initial state (parameters, Adam "
                           "moments, step counter, view cycle and the library's per-view tables reset before each): their spread is noise, not drift",
            **({"ms_per_step_without_kernel_events": (round(m["dt_plain"] / steps * 1e3, 4) if m.get("dt_plain") else None)} if args.full else {}),
            "timed_phase": "steps %d..%d of a training run from the untrained synthetic scene (the heaviest phase: the blended pairs per frame fall as the scene "
                           "trains, see config.per_view[].intersections_blended_first_last_timed_step of a --full line).  Rounds 1-4 timed consecutive windows of a scene that "
                           "kept training (round 4: ~60 steps, 7.5 %% monotone drift between its windows): their views/s are not comparable with this line"
                           % (args.warmup, args.warmup + steps - 1),
            "config": {"workload": "%s: %d splats, %dx%d, SH degree %d, one view per rank per step (BASELINE.json configs[2])" % (args.workload, n, w, h, args.sh_degree),
                       "views": m["nviews"],
                       "view_cycle": ("step k trains view k %% %d; " % m["nviews"]) + ("two cameras 2 units apart in x as crates/brush-bench-test/src/benches.rs:198-220" if m["nviews"] == 2 else
                                                                                   ("one camera replayed" if m["nviews"] == 1 else "an orbit of cameras on a circle of radius 1")),
                       # means over the views of the timed region, counted in an untimed replica of its steps (--full)
                       **({"num_visible": m["nv"], "num_intersections": m["ni"], "per_view": m["per_view"]} if args.full else {}),
                       "near_share": {"min": round(m["near_share_min"], 4), "max": round(m["near_share_max"], 4), "mean": round(m["list_share"], 4),
                                      "of": "every step of the timed windows"} if args.lists == "sliced" else None,
                       "far_slices_queued": m["far_slices_queued"] if args.lists == "sliced" else None,
                       "timed_steps": m["timed_steps"],
                       "lists": ("per-tile depth cuts keyed by view id%s: the near pass lists %.3f of the pairs on average (per tile: what the tile needed at the view's "
                                 "previous visit + a margin), a far pass finishes tiles the forecast missed; image / gradients identical to the exact lists"
                                 % (" (OFF: --no-view-ids, one shared table)" if args.no_view_ids else "", m["list_share"])) if args.lists == "sliced" else "exact (every pair listed and sorted)",
                       "stochastic_terms": "off (--no-noise)" if args.no_noise else "mean noise drawn on the device (Philox-4x32-10, fused into the update launch) + background jitter, as the reference's default step",
                       "parallelism": ("tiles%d: one view split by strips of tile rows (strip-wise loss with 21-px halo exchange + mask-keyed all-reduce of gradients)" % world if tile_mode else
                                       "dp%d over cameras (RCCL all-reduce of gradients%s)" % (world, ", library-owned communicator" if native else ", torch.distributed hook")) if world > 1 else "single GPU"},
            "exchange": ({"mode": args.exchange, "comm": "native" if native else "torch", "algo": args.allreduce, "rows_last_step": st.exchange_rows, "rows_total": n,
                          "per_rank": per_rank, "selfcheck": selfcheck,
                          "stages_us": None, "stages_us_are": "us per step on every rank, HIP events around the stage (10 steps): FlagExchange = visible-flag sum + union "
                                                                         "listing (on the communicator's side stream beside the backward), GradExchange = row gather + all-reduce + scatter "
                                                                         "(or the dense all-reduce), ImageExchange = the strips' halos (tiles only)",
                          "ab": None} if pg is not None else None),
        }
        if args.full:
            out.update(full_figures(m, steps, ms_per_step))
        if loop is not None:
            out["train_loop"] = loop
        if view_runs:
            out["other_view_counts"] = view_runs
        if extra is not None:
            out["non_saturating"] = extra
        if sh3 is not None:
            out["sh3"] = sh3
        if late is not None:
            out["after_growth_stop"] = late
        if centered is not None:
            out["object_centric"] = centered
        if m.get("forward_only"):
            out["forward_only"] = {"workload": "%s, RasterPass::Forward (BASELINE.json configs[1]): packed rgba8 image, no backward state; ms per render call incl. its count readback" % args.workload,
                                   "ms_exact_lists": m["forward_only"]["exact_lists"], "ms_sliced_lists": m["forward_only"]["sliced_lists"],
                                   "near_share": m["forward_only"].get("near_share"), "far_slices_queued": m["forward_only"].get("far_slices_queued")}
        if world == 1 and args.full and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(m["scene"], m["cp"], w, h)
        final_out = out
    # ---- N > 1 side measurements, behind the line's own figures and under a watchdog: a collective that hangs here (the direct
    # all-reduce has never met a second rank on hardware) costs the side measurements, not the line
    exchange_stages, exchange_ab = None, None
    if pg is not None and extras:
        import threading

        def bail():
            if rank == 0 and final_out is not None:
                final_out["exchange"]["ab"] = "side measurements did not finish within 300 s (hung collective?): the line's own figures were taken before them"
                os.write(real_stdout, (json.dumps(final_out) + "\n").encode())
            sys.stderr.write("bench.py: the exchange side measurements hung - leaving without them\n")
            sys.stderr.flush()
            os._exit(0)
        side_timer = threading.Timer(300.0, bail)
        side_timer.daemon = True
        side_timer.start()
    if pg is not None and extras:
        # The first multi-GPU run has to explain itself: (a) what the exchange stages cost per step on every rank
        # (HIP events around FlagExchange / GradExchange / ImageExchange, 10 steps from the same initial state), (b) a 10-step A/B of
        # the exchange modes and of the two all-reduce algorithms (every figure the MAX over the ranks, like the headline)
        import torch.distributed as dist
        # (side measurements: whatever goes wrong here must not cost the run its line — the error is recorded instead; a rank that fails
        #  tells the others, so that nobody waits in a collective the failing rank never enters)
        def all_ok(ok):
            t = torch.tensor([1 if ok else 0], device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MIN)
            return int(t.item()) == 1
        try:
            mp_ = measure(args.workload, 10, 3, True, windows=1)
            mine_st = {k: round(ms / max(c, 1) * 1e3, 2) for k, (ms, c) in mp_["stages"].items() if k in ("FlagExchange", "GradExchange", "ImageExchange", "RasterizeBackwards", "OptimizerStep")}
            ok = True
        except Exception as e:
            mine_st, ok = {"error": repr(e)}, False
        mine_st["rank"] = rank
        exchange_stages = [None] * world
        dist.all_gather_object(exchange_stages, mine_st)
        exchange_ab = {"steps": 10, "what": "ms per step (max over ranks), 10 steps after 3 warm-up steps from the same initial state, per exchange mode x all-reduce algorithm"}
        if all_ok(ok):
            for ex_mode in ("sparse", "dense"):
                for alg in ("ring", "direct"):
                    try:
                        ma = measure(args.workload, 10, 3, False, windows=1, exchange=ex_mode, algo=alg)
                        val, ok = round(ma["dt"] / 10 * 1e3, 4), True
                    except Exception as e:
                        val, ok = "error: %r" % (e,), False
                    exchange_ab["%s_%s" % (ex_mode, alg)] = val
                    if not all_ok(ok):
                        exchange_ab["aborted_after"] = "%s_%s" % (ex_mode, alg)
                        break
                if "aborted_after" in exchange_ab:
                    break

        side_timer.cancel()
        if rank == 0 and final_out is not None:
            final_out["exchange"]["stages_us"] = exchange_stages
            final_out["exchange"]["ab"] = exchange_ab
    if rank == 0 and final_out is not None:
        os.write(real_stdout, (json.dumps(final_out) + "\n").encode())
    if pg is not None:
        import torch.distributed as dist
        # the library's communicator goes first, while RCCL is certainly still alive (left to the interpreter's teardown it was
        # destroyed after torch's process group, in whatever order the garbage collector chose: a crash at exit now and then)
        try:
            torch.cuda.synchronize(dev)
            ctx.comm_destroy()
        except Exception as e:
            print("bench.py: bh_comm_destroy: %s" % (e,), file=sys.stderr)
        dist.barrier()
        dist.destroy_process_group()


KERNEL_STAGE = (("project_forward_kernel", "ProjectSplats"), ("dsort_", "DepthSort"), ("map_gaussians_kernel", "MapGaussiansToIntersect"),
                ("slice_count_kernel", "MapGaussiansToIntersect"), ("radix_", "TileSort"), ("tile_parts_", "TileSort"), ("scan_", "MapGaussiansToIntersect"),
                ("tile_offsets_kernel", "GetTileOffsets"), ("rasterize_backward_kernel", "RasterizeBackwards"), ("rasterize_kernel", "Rasterize"),
                ("loss_fused_forward_kernel", "ImageLoss"), ("loss_fused_backward_kernel", "ImageLossBackward"),
                ("project_backward_kernel", "ProjectBackwards"), ("train_update_kernel", "OptimizerStep"), ("project_visible_kernel", "ProjectVisible"))


def _child_cmd(args, extra):
    """This command again as a child process under rocprofv3: the SAME warm-up and step counts (so that its timed steps are the same
    piece of the same training run as the parent's: VERDICT r4 weak #5 / #6), one window, nothing but the headline measurement and
    the counts of its views (--full without its side measurements: the --pmc passes read `roofline.intersections_blended` of its line)."""
    cmd = [sys.executable, os.path.abspath(__file__), "--steps", str(args.steps), "--warmup", str(args.warmup), "--full", "--no-cpu-baseline", "--no-extra", "--no-pmc",
           "--lists", args.lists, "--views", str(args.views), "--windows", "1"] + extra
    if args.no_noise:
        cmd.append("--no-noise")
    if args.no_view_ids:
        cmd.append("--no-view-ids")
    return cmd


def _timed_dispatch_window(rows, name_key, order_key, warmup, steps):
    """rows of a rocprofv3 per-dispatch CSV -> (lo, hi]: the `order_key` values of the update kernel's dispatches number `warmup` and
    `warmup + steps` (1-based) — every step ends with exactly one train_update_kernel, so the dispatches in between are the timed
    steps of the child's (only) window.  None if the run was shorter than that."""
    upd = sorted(float(r[order_key]) for r in rows if "train_update_kernel" in r[name_key])
    if len(upd) < warmup + steps:
        return None
    return (upd[warmup - 1] if warmup > 0 else -1.0), upd[warmup + steps - 1]


def kernel_trace_inrun(args):
    """Per-stage GPU time from the kernels' own timestamps: one child run of this command under `rocprofv3 --kernel-trace`, and of its
    dispatches only those of the TIMED steps (between the update kernels of step `warmup` and step `warmup + steps`): every library
    kernel's total duration / steps, summed by stage.  The HIP-event stage table of the parent run brackets each stage with two event
    records and is host-bound while it does so (~30 records per step): stages made of several short launches read up to 2x too long
    there.  Returns {steps, stages_us, kernels} or None."""
    import csv
    import glob
    import shutil
    import tempfile
    if os.environ.get("BH_BENCH_PMC_CHILD") == "1" or not shutil.which("rocprofv3"):
        return None
    tmp = tempfile.mkdtemp(prefix="bh_trace_", dir="/tmp")
    env = dict(os.environ, BH_BENCH_PMC_CHILD="1", TMPDIR="/tmp")
    try:
        p = subprocess.run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", tmp, "-o", "trace", "--"] + _child_cmd(args, ["--no-stages"]), cwd="/tmp",
                           env=env, capture_output=True, text=True, timeout=180)
        files = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)
        if p.returncode != 0 or not files:
            return None
        rows = list(csv.DictReader(open(files[0])))
        win = _timed_dispatch_window(rows, "Kernel_Name", "End_Timestamp", args.warmup, args.steps)
        if win is None:
            return None
        per_stage, per_kernel = {}, {}
        t_first, t_last, busy_ns = None, None, 0.0   # the trace's own wall time of the timed steps, and what of it is not kernel time
        for r in rows:
            name = r["Kernel_Name"]
            if "bh::" not in name or not (win[0] < float(r["End_Timestamp"]) <= win[1]):
                continue
            a, b = float(r["Start_Timestamp"]), float(r["End_Timestamp"])
            t_first = a if t_first is None else min(t_first, a)
            t_last = b if t_last is None else max(t_last, b)
            busy_ns += b - a
            short = name.replace("void ", "").replace("bh::", "").split("(")[0]
            us = (float(r["End_Timestamp"]) - float(r["Start_Timestamp"])) / 1e3
            k = per_kernel.setdefault(short, {"us_per_step": 0.0, "avg_us": 0.0, "calls": 0})
            k["us_per_step"] += us
            k["calls"] += 1
        for short, k in per_kernel.items():
            k["avg_us"] = round(k["us_per_step"] / k["calls"], 2)
            k["us_per_step"] = round(k["us_per_step"] / args.steps, 2)
            for key, stage in KERNEL_STAGE:
                if key in short:
                    per_stage[stage] = per_stage.get(stage, 0.0) + k["us_per_step"]
                    break
        span_us = (t_last - t_first) / 1e3 / args.steps if t_first is not None else None
        return {"steps": args.steps, "stages_us": {k: round(v, 2) for k, v in per_stage.items()}, "kernels": per_kernel,
                "wall_us_per_step": (round(span_us, 2) if span_us else None),
                "idle_us_per_step": (round(span_us - busy_ns / 1e3 / args.steps, 2) if span_us else None)}
    except Exception:
        return None
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def pmc_inrun(args):
    """Counter figures of the two blend kernels measured in THIS run: three child runs of this command under `rocprofv3 --pmc <one
    group>` (SQ_INSTS_VALU | FETCH_SIZE | WRITE_SIZE — separate passes; no tracing flags), averaged over the dispatches of the child's
    TIMED steps only (same warm-up and step counts as the parent: the same phase of the same training run).  Returns
    {kernel: {valu_per_blended_isect, hbm_bytes}} or None (no rocprofv3 on PATH, a pass failed, we ARE such a child)."""
    import collections
    import csv
    import glob
    import shutil
    import tempfile
    if os.environ.get("BH_BENCH_PMC_CHILD") == "1" or not shutil.which("rocprofv3"):
        return None
    kernels = ("rasterize_backward_kernel", "rasterize_kernel")
    per_launch, blended = collections.defaultdict(dict), None
    tmp = tempfile.mkdtemp(prefix="bh_pmc_", dir="/tmp")
    env = dict(os.environ, BH_BENCH_PMC_CHILD="1", TMPDIR="/tmp")
    try:
        for counter in ("SQ_INSTS_VALU", "FETCH_SIZE", "WRITE_SIZE"):
            out = os.path.join(tmp, counter)
            p = subprocess.run(["rocprofv3", "--pmc", counter, "--output-format", "csv", "-d", out, "-o", "pmc", "--"] + _child_cmd(args, ["--no-stages"]), cwd="/tmp",
                               env=env, capture_output=True, text=True, timeout=180)
            files = glob.glob(os.path.join(out, "**", "*counter_collection.csv"), recursive=True)
            if p.returncode != 0 or not files:
                return None
            lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
            if lines and blended is None:
                blended = json.loads(lines[-1])["roofline"]["intersections_blended"]
            rows = list(csv.DictReader(open(files[0])))
            win = _timed_dispatch_window(rows, "Kernel_Name", "Dispatch_Id", args.warmup, args.steps)
            if win is None:
                return None
            acc = collections.defaultdict(lambda: [0.0, 0])
            for r in rows:
                if not (win[0] < float(r["Dispatch_Id"]) <= win[1]):
                    continue
                name = r["Kernel_Name"]
                for k in kernels:
                    if ("::" + k + "<") in name or ("::" + k + "(") in name:
                        acc[k][0] += float(r["Counter_Value"])
                        acc[k][1] += 1
            for k, (tot, cnt) in acc.items():
                per_launch[k][counter] = tot / max(cnt, 1)
    except Exception:
        return None
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    res = {}
    for k in kernels:
        d = per_launch.get(k, {})
        e = {}
        if "SQ_INSTS_VALU" in d and blended:
            e["valu_per_blended_isect"] = d["SQ_INSTS_VALU"] / blended
        if "FETCH_SIZE" in d and "WRITE_SIZE" in d:   # KB per launch; FETCH_SIZE under-counts wide reads by 2x on gfx950
            e["hbm_bytes"] = (2.0 * d["FETCH_SIZE"] + d["WRITE_SIZE"]) * 1024.0
        res[k] = e
    return res


def _newest(pattern):
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", pattern)))
    return files[-1] if files else None


def pmc_traffic_bytes(kernel_substr):
    """HBM bytes per launch of `kernel_substr` from the newest profiles/*_hbm_traffic.csv
    (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes, gfx950 x2 read correction applied)."""
    import csv
    f = _newest("*_hbm_traffic.csv")
    if not f:
        return None, None
    for r in csv.DictReader(open(f)):
        if r["kernel"].startswith("void bh::" + kernel_substr) or r["kernel"].startswith(kernel_substr) or ("::" + kernel_substr + "<") in r["kernel"]:
            return float(r["HBM_MB_per_launch_corrected"]) * 1e6, os.path.basename(f)
    return None, None


def valu_per_isect(kernel):
    """VALU wave-instructions per blended (splat, tile): measured (SQ_INSTS_VALU per launch / intersections blended, the newest
    profiles/*_sq_counters.csv written by scripts/collect_profiles.py) or the static ISA count."""
    import csv
    f = _newest("*_sq_counters.csv")
    if f:
        for r in csv.DictReader(open(f)):
            if r["kernel"] == kernel and float(r.get("valu_per_blended_isect") or 0) > 0:
                return float(r["valu_per_blended_isect"]), os.path.basename(f)
    return VALU_PER_ISECT_STATIC[kernel], "static ISA count"


def cpu_baseline(scene, cp, w, h):
    """Full steps of the SAME workload on the CPU oracle (OpenMP over splats/tiles): one warm-up, then the median of 5."""
    import brush_amd as ba
    from brush_amd import synth
    from oracle import bo
    from oracle.trainer import OracleTrainer
    sc = {k: v.copy() for k, v in scene.items()}
    otr = OracleTrainer(bo, ba.TrainConfig(), median_scene_scale=5.0)
    gt = synth.synthetic_gt_packed(w, h, seed=7)
    otr.step(sc, bo.camera(**cp), gt, (0.0, 0.0, 0.0))   # warm-up (page faults, OpenMP pool)
    times = []
    t_all = time.perf_counter()
    for _ in range(5):
        t = time.perf_counter()
        otr.step(sc, bo.camera(**cp), gt, (0.0, 0.0, 0.0))
        times.append(time.perf_counter() - t)
    wall = time.perf_counter() - t_all
    med = sorted(times)[len(times) // 2]
    return {"value": round(1.0 / med, 5), "unit": "views/s", "cores": bo.num_threads(), "kind": "port",
            "sample": "median of 5 full train steps (1 view each, no noise term) of the same workload after 1 warm-up step; %.2f s wall" % wall,
            "what": "C++/OpenMP restatement of Brush's CubeCL kernels (oracle/brush_oracle.cpp); Brush itself has no CPU backend"}


if __name__ == "__main__":
    main()
