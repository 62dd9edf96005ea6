#!/usr/bin/env python3
"""Headline benchmark: forward render of the synthetic 100 000-disc scene at 2048 x 2048 (BASELINE.json
configs[4]), framebuffer row-tiled over N MI355X with one RCCL gather per frame.

    python bench.py --gpus 1 --steps 20 --warmup 3
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \\
        --master-port P bench.py --gpus N --steps K --warmup W

A step is one frame: every rank renders its row slab from primitive arrays already resident in HBM
(prep, binning and render kernels), then the slabs are gathered on rank 0; with more than one rank the gather of
a frame overlaps the render of the next one (two frames in flight).  Rank 0 prints ONE JSON line.
``value`` = frames/s of the whole job; tests/s = primitives x pixels x frames/s (algorithmic pairs, i.e.
what the reference evaluates, whatever the kernel skips).  Total work is fixed as N grows -> "strong".

A plain run does only what that line's headline needs: set-up, warm-up, the --steps timed frames, the line.  --full
adds everything else the benchmark measures and checks (the bit-for-bit check of the timed frames, the CPU baseline,
the half-frame schedule probe, the executed pair tests, the measured link rates).  --dump-outputs DIR writes the
last timed frame's image and depth for output-for-output comparisons of two builds.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import numpy as np
import torch
import torch.distributed as dist

HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
# algorithmic flops of one ray-disc test (arithmetic only, per-primitive constants hoisted) and the
# fp32 vector peak it prices them against
FLOP_PER_DISK_TEST = 17
VALU_F32_PEAK_TFLOPS = 157.3
# What actually bounds the render kernel is vector-instruction issue: tools/ubench_issue.hip (output committed as
# profiles/r02_ubench_issue.txt) gives the cycles per wave-instruction per SIMD for every instruction class the kernel
# uses; the peak below is the rate of its dominant class.
VALU_PEAK_GINSTR_S = 614.4
# newest committed counter file first (tools/collect_pmc.py; one per round)
PMC_FILES = [os.path.join(REPO, "profiles", name) for name in ("r03_pmc.json", "r02_pmc.json")]
MIX_FILE = os.path.join(REPO, "profiles", "r03_valu_mix.json")      # tools/valu_mix.py: the kernel's instruction mix, priced


# --schedule auto = whole frames per stream, always.  The stage schedule (binning of every frame on one stream, render
# kernels on two others) was once picked when the render kernel lasted at least 2.3 times as long as clear + binning
# (equal steady state, 2 % better over a 20-step region with the 105 us kernel, ratio 2.55).  With one-wave workgroups
# and the typed 88 us kernel it is 30 % WORSE at config 5 (0.1068 against 0.0808 ms per frame, 400 steps; 0.1052 against
# 0.0867 over 20 steps) -- and the probe sits at ratio 2.16-2.21, 4 % under the old threshold, so a slightly different
# box would have flipped the default into it.  The probe is still taken and reported with --full (config.schedule_probe);
# --schedule stages remains for measurements.


def load_pmc():
    """Per-launch PMC counters of the render kernel on the default workload, as collected by tools/collect_pmc.py and
    committed under profiles/ together with the commit and the library hash they were taken at.  None when absent."""
    try:
        path = next(p for p in PMC_FILES if os.path.exists(p))
        with open(path) as fh:
            d = json.load(fh)
        k = d["kernels"]["k_render_binned"]
        return {"commit": d.get("commit"), "lib_sha256": d.get("lib_sha256"), "file": os.path.relpath(path, REPO),
                # HBM bytes: WRITE_SIZE + 2 x FETCH_SIZE (KiB units; the guide's gfx950 correction for the read side)
                "traffic_bytes": (k["WRITE_SIZE"] + 2.0 * k["FETCH_SIZE"]) * 1024.0,
                "valu_wave_instr": float(k["SQ_INSTS_VALU"])}
    except Exception:                                       # noqa: BLE001 -- no file, no constants
        return None


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--mode", default="auto", choices=["auto", "exact", "fast", "binned"])
    ap.add_argument("--prims", type=int, default=100_000)
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--height", type=int, default=2048)
    ap.add_argument("--inflight", type=int, default=0,
                    help="frames in flight: each has its own stream and scratch, so the binning kernels of one frame "
                         "overlap the render kernel of another.  Default 3 (measured: 1 -> 7.7k, 2 -> 11.9k, 3 -> 12.2k, "
                         "4 -> 10.7k, 5 -> 12.1k, 6 -> 12.3k frames/s on one MI355X)")
    ap.add_argument("--schedule", default="auto", choices=["auto", "frames", "stages", "render-only", "bin-only"],
                    help="single process: 'frames' = each frame whole on its own stream (--inflight of them); 'stages' = "
                         "one stream for every frame's binning kernels, --render-streams for the render kernels (same "
                         "steady state, 2 %% faster over a 20-step timed region: the streams do not start in lockstep); "
                         "auto = stages when the frames are binned, graphs are on, at least three frames are in flight and "
                         "the render kernel of a whole frame takes at least twice as long as its binning (timed once), "
                         "else frames")
    ap.add_argument("--render-streams", type=int, default=2, help="--schedule stages: streams the render kernels alternate over")
    ap.add_argument("--bin-priority", action="store_true", help="--schedule stages: the binning stream gets the higher priority")
    ap.add_argument("--flat-priority", action="store_true", help="--schedule stages: do not raise the render streams' priority")
    ap.add_argument("--gather", default="alltoall", choices=["alltoall", "root0"],
                    help="multi-GPU collection: batches of N frames, frame k assembled on rank k by one all-to-all "
                         "(default), or one gather per frame to rank 0")
    ap.add_argument("--graph", default="auto", choices=["auto", "on", "off"],
                    help="replay each frame's kernel sequence (clear, prep-and-bin, render) as one "
                         "hipGraph per output slot instead of three launches; auto = on for a single process (eager if "
                         "capture fails), off when a process group is in use")
    ap.add_argument("--as-rank", default=None, metavar="R/P",
                    help="single-process rehearsal: render only the row slab rank R of a P-rank job would own (no "
                         "collection), to size the per-rank cost of the multi-GPU path on one GPU")
    ap.add_argument("--parallelism", default="rows", choices=["rows", "frames"],
                    help="rows (the metric's definition): every frame is row-tiled over the ranks and collected.  "
                         "frames: every rank renders whole frames of its own, nothing is collected -- the axis the "
                         "reference's callers actually have (SURVEY 8f row f4); reported as weak scaling")
    ap.add_argument("--batch-call", default="auto", choices=["auto", "on", "off"],
                    help="multi-GPU batched collection: render a rank's slab of all P frames of a batch with ONE "
                         "library call (srh_render_views: every kernel launched once per batch) instead of P calls; "
                         "auto = on (rehearsed with --as-rank against per-frame graph replays, which multi-GPU runs "
                         "cannot use: 34 vs 45 us per frame at P = 8, 56 vs 57 at P = 4, 73 vs 71 at P = 2)")
    ap.add_argument("--owner-frac", type=float, default=0.0,
                    help="--slabs owner: the fraction of a frame's rows rendered by the rank that assembles it; "
                         "0 = the others render 128 rows each (0.9375 at 2 ranks, 0.8125 at 4 for 2048 rows)")
    ap.add_argument("--tile-row-cost", type=float, default=10.0,
                    help="--slabs cost: fixed cost of a tile besides its list entries, in entries (an empty tile still "
                         "stores its background: measured ~3 us against ~29 us for a median tile of ~90 entries)")
    ap.add_argument("--slabs", default="auto", choices=["auto", "contiguous", "balanced", "owner", "cost"],
                    help="rows of a rank: one contiguous slab, or (batched collection, H %% 2P == 0) two half-slabs, "
                         "g and P+g of 2P, so that a scene that is densest in the middle loads every rank alike.  "
                         "auto = contiguous: rehearsed with --as-rank, the balanced form evens the ranks out (26-40 us "
                         "instead of 9-34 us at P = 8) but its doubled per-view fixed work makes the slowest rank "
                         "slower (40 vs 34 us at P = 8, 59 vs 56 at P = 4).  owner = owner-weighted slabs "
                         "(dist.owner_slabs): the rank that assembles a frame renders --owner-frac of it, so that less "
                         "of the frame crosses the xGMI links; auto picks it at 2 and 4 ranks, where an equal split is "
                         "bound by the links (four times over at 2 ranks) and the middle slabs are the busiest")
    ap.add_argument("--force-dist", action="store_true",
                    help="rehearsal: create the RCCL process group and use the multi-GPU frame collection even with "
                         "one rank (exercises the collective, stream and graph plumbing on a one-GPU box)")
    ap.add_argument("--full", action="store_true",
                    help="besides the headline, run everything else the benchmark measures and checks: the bit-for-bit "
                         "check (--check), the CPU baseline, the half-frame schedule probe, the executed pair tests "
                         "and, with several ranks, the measured link rates.  Off: only what the headline needs")
    ap.add_argument("--check", dest="check", action="store_true", default=None,
                    help="(default with --full) after the timed loop compare every output slot / collected frame on this "
                         "rank, bit for bit, with a fresh eager render of the same rows and exit non-zero on a mismatch "
                         "(stream / graph / collective ordering self-test; outside the timed region)")
    ap.add_argument("--no-check", dest="check", action="store_false")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps write what the last timed frame computed as DIR/image.npy (k, 3), "
                         "DIR/depth.npy (k,) and DIR/hit.npy (k,: 1 hit, 0 nothing hit, where depth is then 0 instead "
                         "of +inf), float32, at k pixels drawn with a fixed seed (at most 2^21, all of them for smaller "
                         "frames), and their row-major pixel numbers as DIR/pixel_index.npy (float64); single-process "
                         "runs")
    ap.add_argument("--allow-fallback", action="store_true",
                    help="multi-GPU: when the default collection schedule fails its bit-for-bit check and the headline "
                         "falls back to the literal gather-to-rank-0 form, exit 0 anyway (the line still carries "
                         "check_failed: true).  Without this flag such a run prints its line and exits 3")
    ap.add_argument("--warmup-ms", type=float, default=150.0,
                    help="after the --warmup steps keep submitting untimed frames until this much wall time has passed "
                         "since the first warm-up frame, so that a short run is timed at ramped clocks")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: leave the CPU baseline out")
    ap.add_argument("--cpu-pixels", type=int, default=4096, help="pixels in the CPU-baseline sample (about 14 s of numpy)")
    args = ap.parse_args()
    if args.check is None:
        args.check = args.full
    return args


def cpu_baseline(scene, prims, width, height, npix):
    """The oracle (numpy restatement of the reference's CPU path) timed on this host, on a bounded
    sample of the same workload: `npix` consecutive pixels (row-major) centred on the middle image row against all
    primitives.  numpy's elementwise kernels run on one core."""
    from oracle import np_oracle                       # checker / baseline only -- never the product path
    from surf_renderer_amd.scene import scene_to_numpy
    sc = scene_to_numpy(scene, round_fp32=True)
    p0 = (height // 2) * width + (width - npix) // 2
    t0 = time.perf_counter()
    np_oracle.render(sc, tile=64, window=(p0, p0 + npix))
    dt = time.perf_counter() - t0
    tests = float(prims) * npix
    tps = tests / dt
    return {"value": tps / (float(prims) * width * height), "unit": "frames/s", "cores": 1,
            "kind": "port", "mtests_per_s": tps / 1e6,
            "extrapolated_s_per_frame": float(prims) * width * height / tps,
            "host_cpus": os.cpu_count(),
            "sample": f"{npix} consecutive pixels around the middle of the image x {prims} discs ({tests:.3g} tests, "
                      f"{dt:.1f} s), oracle/np_oracle.py fp64, pixel tile 64; frames/s extrapolated"}


DUMP_PIXELS = 1 << 21          # x (12 + 4 + 4 + 8) bytes: at most 59 MB of .npy files


def dump_outputs(out_dir, slab, width, row0):
    """--dump-outputs: what a caller of the timed path receives for one frame, the image (rows, W, 3) and depth (rows, W)
    views of its output slab, at a fixed, seeded sample of the pixels (every pixel of a small frame).  The library's
    depth is +inf where nothing is hit; the files hold only finite numbers, so that is written as hit = 0 and depth = 0
    (a hit lies beyond the near clip, so 0 is no depth of a hit).  Anything else that is not finite stays as it is."""
    from surf_renderer_amd.pipeline import slab_views
    image, depth = slab_views(slab, width)
    n = depth.numel()
    idx = np.arange(n) if n <= DUMP_PIXELS else \
        np.sort(np.random.default_rng(0).choice(n, DUMP_PIXELS, replace=False))
    at = torch.from_numpy(idx).to(slab.device)
    d = depth.reshape(n)[at].cpu().numpy()
    miss = d == np.inf
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "image.npy"), image.reshape(n, 3)[at].cpu().numpy())
    np.save(os.path.join(out_dir, "depth.npy"), np.where(miss, np.float32(0), d))
    np.save(os.path.join(out_dir, "hit.npy"), (~miss).astype(np.float32))
    np.save(os.path.join(out_dir, "pixel_index.npy"), (idx + row0 * width).astype(np.float64))   # row-major, whole frame


def literal_root0_leg(args, buf, cam, device, rank, world, W, H):
    """The metric's literal form, timed beside the default schedule so that one multi-GPU run answers both questions:
    equal contiguous row slabs, every frame assembled on rank 0 by ONE gather per frame (dist.gather_rows), eager
    launches, two frames in flight (the gather of one overlaps the render of the next).  Same warm-up rule, exactly
    --steps timed frames, max over ranks; rank 0 checks its assembled frames against an eager full-frame render."""
    from surf_renderer_amd import renderer
    from surf_renderer_amd.dist import gather_rows, row_slab
    from surf_renderer_amd.pipeline import slab_views
    r0, r1 = row_slab(H, rank, world)
    n_buf = 2
    streams = [torch.cuda.Stream(device) for _ in range(n_buf)]
    scratch = [buf.new_workspace(W, H) for _ in range(n_buf)]
    frames = [torch.empty((H, 4 * W), dtype=torch.float32, device=device) if rank == 0 else None for _ in range(n_buf)]
    slabs = [frames[b][r0:r1] if rank == 0 else torch.empty((r1 - r0, 4 * W), dtype=torch.float32, device=device)
             for b in range(n_buf)]
    pending = [None] * n_buf
    count = [0]

    def step():
        b = count[0] % n_buf
        count[0] += 1
        with torch.cuda.stream(streams[b]):
            if pending[b] is not None:
                pending[b].wait()
                pending[b] = None
            image, depth = slab_views(slabs[b], W)
            renderer.render_buffers(buf, cam, rows=(r0, r1), mode=args.mode, out=(image, depth, None), workspace=scratch[b])
            pending[b] = gather_rows(slabs[b], frames[b], H, dst=0, async_op=True)

    def fence():
        for b in range(n_buf):
            if pending[b] is not None:
                with torch.cuda.stream(streams[b]):
                    pending[b].wait()
                pending[b] = None
        torch.cuda.synchronize(device)
        dist.barrier()
        torch.cuda.synchronize(device)

    t_w = time.perf_counter()
    for _ in range(max(args.warmup, 2)):
        step()
    fence()
    spent = torch.tensor([time.perf_counter() - t_w], dtype=torch.float64, device=device)
    dist.all_reduce(spent, op=dist.ReduceOp.MAX)
    per = max(float(spent.item()) / max(args.warmup, 2), 2e-5)
    extra = int(min(max((args.warmup_ms * 1e-3 - float(spent.item())) / per, 0), 5000))
    for _ in range(extra):
        step()
    fence()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    fence()
    el = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=device)
    dist.all_reduce(el, op=dist.ReduceOp.MAX)
    ok = torch.ones(1, device=device)
    if rank == 0 and args.check:
        ref = torch.empty((H, 4 * W), dtype=torch.float32, device=device)
        renderer.render_buffers(buf, cam, rows=(0, H), mode=args.mode, out=(*slab_views(ref, W), None))
        torch.cuda.synchronize(device)
        for b in range(min(n_buf, count[0])):
            if not torch.equal(frames[b].view(torch.int32), ref.view(torch.int32)):
                ok.zero_()
    dist.all_reduce(ok, op=dist.ReduceOp.MIN)
    el = float(el.item())
    if float(ok.item()) < 1.0:
        # not fatal by itself: the caller keeps the default schedule's (checked) result and shows this leg as failed
        if rank == 0:
            print("[bench] literal gather-to-rank-0 leg: an assembled frame differs from the eager full-frame render",
                  file=sys.stderr)
        return {"failed": True, "value": args.steps / el, "unit": "frames/s", "ms_per_step": 1e3 * el / args.steps,
                "collection": "gather to rank 0 per frame (one collective per frame)",
                "check": "FAILED: an assembled frame differs from the eager full-frame render; not a result"}
    return {"value": args.steps / el, "unit": "frames/s", "ms_per_step": 1e3 * el / args.steps,
            "collection": "gather to rank 0 per frame (one collective per frame)",
            "rows_per_rank": "one contiguous slab, equal split", "launch": "eager", "frames_in_flight": n_buf,
            "check": "rank 0's assembled frames equal an eager full-frame render bit for bit" if args.check else "off"}


def ranks_agree_failed(bad, rank, device, what):
    """True on every rank when the check failed on any rank (one all-reduce; every rank must call it).
    SRH_BENCH_INJECT_CHECK_FAIL=<rank> makes that rank report a failure (rehearsal of the fallback)."""
    if os.environ.get("SRH_BENCH_INJECT_CHECK_FAIL") == str(rank):
        bad = True
    flag = torch.tensor([0.0 if bad else 1.0], device=device)
    if bad:
        print(f"[bench] rank {rank}: check FAILED: {what}", file=sys.stderr)
    dist.all_reduce(flag, op=dist.ReduceOp.MIN)
    return float(flag.item()) < 1.0


def measure_exchange(device, rank, world, W, H, reps=10):
    """Measured rate of the two collections on this node's links, nothing else running: bytes that cross the links per
    rank divided by the wall time of the collective alone (max over ranks).  all-to-all of one batch of `world` frames
    (every rank sends and receives (P-1)/P of a frame); gather of one frame to rank 0 (rank 0 receives (P-1)/P of it)."""
    from surf_renderer_amd.dist import exchange_frames, gather_rows, row_slab
    h = H // world
    out = {}
    if H % world == 0:
        send = torch.rand((world, h, 4 * W), dtype=torch.float32, device=device)
        recv = torch.empty_like(send)
        for _ in range(3):
            exchange_frames(send, recv)
        torch.cuda.synchronize(device)
        dist.barrier()
        t0 = time.perf_counter()
        for _ in range(reps):
            exchange_frames(send, recv)
        torch.cuda.synchronize(device)
        t = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        ms = 1e3 * float(t.item()) / reps
        sent = (world - 1) * h * 4 * W * 4.0
        out["all_to_all_batch"] = {"ms": ms, "bytes_sent_per_rank": sent, "GB_s_per_rank_each_way": sent / (ms * 1e-3) / 1e9}
    r0, r1 = row_slab(H, rank, world)
    slab = torch.rand((r1 - r0, 4 * W), dtype=torch.float32, device=device)
    full = torch.empty((H, 4 * W), dtype=torch.float32, device=device) if rank == 0 else None
    for _ in range(3):
        gather_rows(slab, full, H, dst=0)
    torch.cuda.synchronize(device)
    dist.barrier()
    t0 = time.perf_counter()
    for _ in range(reps):
        gather_rows(slab, full, H, dst=0)
    torch.cuda.synchronize(device)
    t = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=device)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    ms = 1e3 * float(t.item()) / reps
    recvd = (H - (row_slab(H, 0, world)[1] - row_slab(H, 0, world)[0])) * 4 * W * 4.0
    out["gather_to_rank0_frame"] = {"ms": ms, "bytes_received_by_rank0": recvd,
                                    "GB_s_into_rank0": recvd / (ms * 1e-3) / 1e9 if recvd else None}
    return out


def main():
    args = parse()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        if world == 1 and args.gpus > 1:
            raise SystemExit("launch multi-GPU runs with torch.distributed.run (one rank per GPU)")
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU")
    if os.environ.get("SRH_BENCH_SINGLE_DEVICE"):      # rehearsal on a one-GPU box: every rank shares device 0
        local = 0
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    use_dist = world > 1 or args.force_dist
    if use_dist:
        if args.force_dist and "MASTER_ADDR" not in os.environ:
            os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT="29533", RANK="0", WORLD_SIZE="1")
        # SRH_BENCH_BACKEND=gloo (with SRH_BENCH_SINGLE_DEVICE=1): rehearsal of the multi-rank schedule on a one-GPU box,
        # where RCCL refuses two ranks on one device
        backend = os.environ.get("SRH_BENCH_BACKEND", "nccl")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=device)
        else:
            dist.init_process_group(backend)

    from surf_renderer_amd import _lib, renderer, synthetic
    from surf_renderer_amd.dist import (FrameBatcher, balanced_slabs, exchange_frames, exchange_frames_uneven, gather_rows,
                                        owner_slabs, row_slab)

    W, H, M = args.width, args.height, args.prims
    scene = synthetic.disk_cloud_scene(M, W, H)          # same seed on every rank -> identical replicas
    buf = renderer.flatten_scene(scene, device)
    cam = renderer.camera_struct(scene["camera"])
    frames_par = args.parallelism == "frames" and world > 1
    r0, r1 = (0, H) if frames_par else row_slab(H, rank, world)
    if args.as_rank:
        er, ep = (int(t) for t in args.as_rank.split("/"))
        r0, r1 = row_slab(H, er, ep)
    # --slabs cost: contiguous slabs of equal WORK, from the bin lengths of one probe frame (every rank computes the same
    # partition from its identical scene replica; nothing is communicated).  Default at 8 ranks: with equal slabs the
    # middle ranks see twice the candidates of the outer ones and set the pace (profiles/r02_rank_rehearsal.txt).
    cost_parts = None
    n_parts = int(args.as_rank.split("/")[1]) if args.as_rank else world
    if not frames_par and n_parts > 1 and (args.slabs == "cost" or (args.slabs == "auto" and n_parts >= 8)) and \
            args.mode in ("auto", "binned"):
        from surf_renderer_amd.dist import cost_weighted_slabs
        stats = renderer.bin_statistics(buf, cam)
        cost_parts = cost_weighted_slabs(stats["tile_row_cost"], H, n_parts,
                                         per_tile_row=args.tile_row_cost * ((W + 15) // 16))
        r0, r1 = cost_parts[int(args.as_rank.split("/")[0]) if args.as_rank else rank]
    h = r1 - r0

    # Framebuffer layout: (rows, 4W) fp32 per slab -- [W x rgb | W x depth] per row -- so one transfer moves both.
    # `inflight` frames are in flight on their own streams with their own scratch (binning of one frame overlaps the
    # render of another).
    #   1 rank    frames are rendered in place.
    #   P ranks   frames are gathered in BATCHES of P with rotating roots: frame k of a batch is assembled on rank k
    #             by one all-to-all (surf_renderer_amd.dist.exchange_frames) -- per frame the same bytes as a gather to
    #             rank 0, but spread over every rank's xGMI links; two batches are buffered so the exchange of one
    #             overlaps the rendering of the next.  (--gather root0: the plain one-gather-per-frame to rank 0.)
    n_str = args.inflight if args.inflight > 0 else 3
    streams = [torch.cuda.Stream(device) for _ in range(n_str)]
    scratch = [buf.new_workspace(W, H) for _ in range(n_str)]
    equal_slabs = H % world == 0
    batched = use_dist and equal_slabs and args.gather == "alltoall" and not frames_par
    if batched:
        # pre-flight: one tiny exchange; if this stack cannot do it, every rank falls back to the gather to rank 0
        ok = torch.ones(1, device=device)
        try:
            probe = torch.arange(world * 4, dtype=torch.float32, device=device).reshape(world, 1, 4) + 100.0 * rank
            got = torch.empty_like(probe)
            exchange_frames(probe, got)
            torch.cuda.synchronize(device)
            want = torch.stack([torch.arange(4, dtype=torch.float32, device=device) + 4 * rank + 100.0 * g
                                for g in range(world)]).reshape(world, 1, 4)
            if not torch.equal(got, want):
                ok.zero_()
        except Exception as exc:                          # noqa: BLE001 -- any failure means "do not use it"
            print(f"[bench] rank {rank}: all-to-all pre-flight failed ({exc!r})", file=sys.stderr)
            ok.zero_()
        dist.all_reduce(ok, op=dist.ReduceOp.MIN)
        if float(ok.item()) < 1.0:
            if rank == 0:
                print("[bench] all-to-all collection unavailable: falling back to one gather per frame to rank 0",
                      file=sys.stderr)
            batched = False
    # the rows this rank renders: one slab, or two half-slabs (batched collection only; the collected frame is then the
    # concatenation, in rank order, of [half-slab g | half-slab P+g])
    balanced = batched and not args.as_rank and args.slabs == "balanced" and H % (2 * world) == 0
    pieces = balanced_slabs(H, rank, world) if balanced else [(r0, r1)]
    # owner-weighted slabs (batched collection only): my rows of the frame that rank k assembles differ per k
    owner = batched and not args.as_rank and world > 1 and \
        (args.slabs == "owner" or (args.slabs == "auto" and world <= 4 and H >= 256 * world) or cost_parts is not None)
    if owner:
        # pre-flight of the unequal-split exchange; if this stack cannot do it, every rank keeps the equal slabs
        ok = torch.ones(1, device=device)
        try:
            sr = [3 if k == rank else 1 for k in range(world)]
            src = torch.cat([torch.full((sr[k], 4), 100.0 * rank + k, device=device) for k in range(world)])
            dst = torch.empty((sum(sr), 4), dtype=torch.float32, device=device)
            exchange_frames_uneven(src, dst, sr, sr)
            torch.cuda.synchronize(device)
            want = torch.cat([torch.full((sr[g], 4), 100.0 * g + rank, device=device) for g in range(world)])
            if not torch.equal(dst, want):
                ok.zero_()
        except Exception as exc:                          # noqa: BLE001
            print(f"[bench] rank {rank}: unequal all-to-all pre-flight failed ({exc!r})", file=sys.stderr)
            ok.zero_()
        dist.all_reduce(ok, op=dist.ReduceOp.MIN)
        if float(ok.item()) < 1.0:
            if rank == 0:
                print("[bench] unequal-split exchange unavailable: equal slabs", file=sys.stderr)
            owner = False
    if owner and cost_parts is not None:
        rows_all = [cost_parts] * world                # the same work-balanced partition for every frame of a batch
        my_rows = [rows_all[k][rank] for k in range(world)]
        send_rows = [b_ - a for a, b_ in my_rows]
        recv_rows = [b_ - a for a, b_ in rows_all[rank]]
        pieces = [my_rows[rank]]
    elif owner:
        owner_frac = args.owner_frac if args.owner_frac > 0 else 1.0 - (world - 1) * min(128, H // (2 * world)) / H
        rows_all = owner_slabs(H, world, owner_frac)
        my_rows = [rows_all[k][rank] for k in range(world)]
        send_rows = [b_ - a for a, b_ in my_rows]
        recv_rows = [b_ - a for a, b_ in rows_all[rank]]
        pieces = [my_rows[rank]]                   # the launch the event pairs bracket: my own frame's tall slab
    main = torch.cuda.current_stream(device)
    # the render kernel's own duration (roofline) comes from event pairs around it on every `ev_every`-th timed
    # step; those steps launch eagerly, the others replay graphs
    ev_every = 1 if args.graph == "off" else 8
    if owner:
        # frames go out one library call each; every 4th batch the tall slab (my own frame's) carries the event pair
        events = [_lib.EventPair() if (i % world == rank and (i // world) % 4 == 0) else None for i in range(args.steps)]
    elif batched and args.batch_call != "off":
        # whole batches are one library call; every 8th batch is rendered frame by frame with the events
        events = [_lib.EventPair() if (i // world) % 8 == 0 else None for i in range(args.steps)]
    else:
        # never the first frames of the timed region: an eager frame there (three launches instead of one replay) delays
        # the start of a pipeline that a short run has only a few frames to amortise
        events = [_lib.EventPair() if i % ev_every == ev_every // 2 else None for i in range(args.steps)]
    counter = [0]
    pipe, schedule, halves = None, "frames", None

    graphs = {}
    # Graph replay is the default on the single-process path only; --graph on asks for it with a process group too.
    graph_state = {"on": args.graph == "on" or (args.graph == "auto" and not use_dist), "captured": 0}
    # (Round 1's GPU memory fault of `--force-dist --graph on` is explained and fixed -- DESIGN.md section 5: the
    # hipMemsetAsync node of a captured frame did not take effect in replays beside the process group, so bin counters
    # accumulated and k_bin_fill (since replaced by the one-pass binner, whose slot index is bounded by the bin's
    # capacity) wrote outside the workspace; the counters are now zeroed by a kernel.  Multi-GPU runs still default to eager launches until graphs have run on real multi-rank hardware.)

    def enqueue(key, stream, image, depth, ws, ev, rows=None):
        """One frame's kernels on `stream`: replay of the hipGraph captured for this (output slot, scratch) pair,
        eager launches the first time, when a timing event pair is to be recorded, or when graphs are off."""
        if graph_state["on"] and ev is None:
            g = graphs.get(key)
            if g is None:
                try:
                    g = torch.cuda.CUDAGraph()
                    # thread_local: the process group's watchdog thread may query events while we capture
                    with torch.cuda.graph(g, stream=stream, capture_error_mode="thread_local"):
                        renderer.render_buffers(buf, cam, rows=rows or (r0, r1), mode=args.mode,
                                                out=(image, depth, None), workspace=ws)
                    graphs[key] = g
                    graph_state["captured"] += 1
                except Exception as exc:                      # capture unsupported here: stay eager, say so
                    if args.graph == "on":
                        raise
                    print(f"[bench] hipGraph capture failed ({exc!r}); eager launches", file=sys.stderr)
                    graph_state["on"] = False
                    g = None
            if g is not None:
                with torch.cuda.stream(stream):
                    g.replay()
                return
        with torch.cuda.stream(stream):
            renderer.render_buffers(buf, cam, rows=rows or (r0, r1), mode=args.mode, out=(image, depth, None),
                                    events=ev, workspace=ws)

    def views(slab):
        hh = slab.shape[0]
        return (slab.as_strided((hh, W, 3), (4 * W, 3, 1), slab.storage_offset()),
                slab.as_strided((hh, W), (4 * W, 1), slab.storage_offset() + 3 * W))

    if batched and owner:
        n_bat = 2

        def render_slot(i, slot, ev):
            k = i % world
            enqueue((i // world % n_bat, k, 0), streams[k % n_str], *views(slot), scratch[k % n_str], ev, rows=my_rows[k])

        def before_exchange():
            for s_ in streams:
                main.wait_stream(s_)               # every slab of the batch is rendered

        def after_reuse_wait():
            for s_ in streams:
                s_.wait_stream(main)               # main waited for the exchange that used this buffer

        batcher = FrameBatcher(world, (0, 4 * W), torch.float32, device, render_slot, before_exchange,
                               after_reuse_wait, n_batches=n_bat, send_rows=send_rows, recv_rows=recv_rows)
        send, recv = batcher.send, batcher.recv
        # work-balanced slabs are the same rows for every frame of a batch: the rank's slab of all P frames is ONE
        # library call (srh_render_views), as with equal slabs; frames with timing events still go out one by one
        one_call = cost_parts is not None and args.batch_call != "off"
        views_ws = [None] * n_bat
        pending_evs = []

        def render_batch(first, send_b):
            st = streams[(first // world) % n_str]
            b = (first // world) % n_bat
            img = send_b.as_strided((world, h, W, 3), (h * 4 * W, 4 * W, 3, 1), 0)
            dep = send_b.as_strided((world, h, W), (h * 4 * W, 4 * W, 1), 3 * W)
            with torch.cuda.stream(st):
                views_ws[b] = renderer.render_views_buffers(buf, [cam] * world, img, dep, rows=(0, h),
                                                            view_row0=[r0] * world, workspace=views_ws[b],
                                                            image_row_stride=4 * W, depth_row_stride=4 * W)

        def step(ev=None):
            counter[0] += 1
            if not one_call:
                batcher.submit(ev)
                return
            pending_evs.append(ev)
            if len(pending_evs) == world:
                if any(e is not None for e in pending_evs):
                    for e in pending_evs:
                        batcher.submit(e)
                else:
                    batcher.submit_batch(render_batch)
                pending_evs.clear()

        def fence():
            for e in pending_evs:                      # a partial last batch goes frame by frame
                batcher.submit(e)
            pending_evs.clear()
            batcher.flush()
            torch.cuda.synchronize(device)
            dist.barrier()
            torch.cuda.synchronize(device)
    elif batched:
        n_bat = 2

        def render_slot(i, slot, ev):
            k = i % world
            at = 0
            for j, (a, b_) in enumerate(pieces):   # the slot holds this rank's pieces one after the other
                part = slot[at:at + (b_ - a)]
                enqueue((i // world % n_bat, k, j), streams[k % n_str], *views(part), scratch[k % n_str],
                        ev if j == 0 else None, rows=(a, b_))
                at += b_ - a

        def before_exchange():
            for s_ in streams:
                main.wait_stream(s_)               # every slab of the batch is rendered

        def after_reuse_wait():
            for s_ in streams:
                s_.wait_stream(main)               # main waited for the exchange that used this buffer

        batcher = FrameBatcher(world, (h, 4 * W), torch.float32, device, render_slot, before_exchange,
                               after_reuse_wait, n_batches=n_bat)
        send, recv = batcher.send, batcher.recv

        # One library call per batch: the P frames of a batch are the "views" of srh_render_views, rendered straight
        # into the send buffer -- one set of launches per batch instead of one per frame, which is what a rank's small slab needs
        # (its kernels are short; per-frame launches leave the GPU idle between them).  Every `ev_every`-th batch is
        # still rendered frame by frame with the timing events around the render kernel.
        batch_call = args.batch_call != "off"
        views_ws = [None] * n_bat
        npc = len(pieces)                          # views per frame: the rank's pieces, all of ph rows
        ph = pieces[0][1] - pieces[0][0]
        cams = [cam] * (world * npc)
        view_row0 = [a for _ in range(world) for a, _ in pieces]

        def render_batch(first, send_b):
            st = streams[(first // world) % n_str]
            b = (first // world) % n_bat
            img = send_b.as_strided((world * npc, ph, W, 3), (ph * 4 * W, 4 * W, 3, 1), 0)
            dep = send_b.as_strided((world * npc, ph, W), (ph * 4 * W, 4 * W, 1), 3 * W)
            with torch.cuda.stream(st):
                views_ws[b] = renderer.render_views_buffers(buf, cams, img, dep, rows=(0, ph), view_row0=view_row0,
                                                            workspace=views_ws[b], image_row_stride=4 * W,
                                                            depth_row_stride=4 * W)

        def step_batch(evs):
            """Render and submit one whole batch; `evs` = per-frame event pairs (or Nones)."""
            if not batch_call or any(e is not None for e in evs):
                for e in evs:
                    batcher.submit(e)
            else:
                batcher.submit_batch(render_batch)

        pending_evs = []

        def step(ev=None):
            pending_evs.append(ev)
            if len(pending_evs) == world:
                step_batch(list(pending_evs))
                pending_evs.clear()
            counter[0] += 1

        def drain_partial():
            for e in pending_evs:                  # a partial last batch goes frame by frame
                batcher.submit(e)
            pending_evs.clear()

        def fence():
            drain_partial()
            batcher.flush()
            torch.cuda.synchronize(device)
            dist.barrier()
            torch.cuda.synchronize(device)
    elif args.as_rank and args.batch_call == "on":
        # rehearsal of a rank's batched rendering on one GPU: its slab of P frames per library call, no collection
        er, ep = (int(t) for t in args.as_rank.split("/"))
        rp = balanced_slabs(H, er, ep) if (args.slabs == "balanced" and H % (2 * ep) == 0) else [(r0, r1)]
        npc_r, ph_r = len(rp), rp[0][1] - rp[0][0]
        row0_r = [a for _ in range(ep) for a, _ in rp]
        bufs = [torch.empty((ep, h, 4 * W), dtype=torch.float32, device=device) for _ in range(n_str)]
        wss = [None] * n_str
        acc = [0]

        def step(ev=None):
            acc[0] += 1
            counter[0] += 1
            if acc[0] % ep:
                return
            j = (acc[0] // ep) % n_str
            img = bufs[j].as_strided((ep * npc_r, ph_r, W, 3), (ph_r * 4 * W, 4 * W, 3, 1), 0)
            dep = bufs[j].as_strided((ep * npc_r, ph_r, W), (ph_r * 4 * W, 4 * W, 1), 3 * W)
            with torch.cuda.stream(streams[j]):
                wss[j] = renderer.render_views_buffers(buf, [cam] * (ep * npc_r), img, dep, rows=(0, ph_r),
                                                       view_row0=row0_r, workspace=wss[j],
                                                       image_row_stride=4 * W, depth_row_stride=4 * W)

        def fence():
            torch.cuda.synchronize(device)
        n_buf, slabs = 0, []
    elif not use_dist:
        # single process: surf_renderer_amd.pipeline.FramePipeline (the same object tests/test_hip_pipeline.py checks)
        from surf_renderer_amd.pipeline import FramePipeline
        one_slab = None
        if os.environ.get("SRH_BENCH_ONE_SLAB"):     # diagnostic: every frame in flight writes the same output slab
            one_slab = [torch.empty((r1 - r0, 4 * W), dtype=torch.float32, device=device)] * \
                (n_str * int(os.environ.get("SRH_BENCH_ROTATE", "1")))
        rotate = int(os.environ.get("SRH_BENCH_ROTATE", "1"))

        def make_pipe(schedule):
            return FramePipeline(buf, cam, rows=(r0, r1), n_inflight=n_str, mode=args.mode, graphs=graph_state["on"],
                                 slabs=one_slab, strict_graphs=args.graph == "on", schedule=schedule,
                                 render_streams=args.render_streams, prioritise_render=not args.flat_priority,
                                 prioritise_bin=args.bin_priority, rotate=rotate)
        def halves_ms():
            """One eager frame's two halves (binning kernels, render kernel), timed alone on the current stream."""
            ws = buf.new_workspace(W, H)
            tmp = torch.empty((r1 - r0, 4 * W), dtype=torch.float32, device=device)
            image, depth = views(tmp)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            for it in range(3):                        # two warm passes, the third one is timed
                if it == 2:
                    ev[0].record()
                renderer.render_buffers(buf, cam, rows=(r0, r1), mode=args.mode, out=(image, depth, None), workspace=ws,
                                        stages=_lib.STAGE_BIN)
                if it == 2:
                    ev[1].record()
                renderer.render_buffers(buf, cam, rows=(r0, r1), mode=args.mode, out=(image, depth, None), workspace=ws,
                                        stages=_lib.STAGE_RENDER)
            ev[2].record()
            torch.cuda.synchronize(device)
            return ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2])

        halves = None
        schedule = args.schedule
        if schedule == "auto":
            # whole frames per stream (see the note at the top); one frame's halves are timed for the report only
            schedule = "frames"
            if args.full and args.mode in ("auto", "binned") and graph_state["on"] and rotate == 1 and n_str >= 3 and \
                    (r0, r1) == (0, H):
                try:                                   # the library refuses split frames that are not binned
                    bin_ms, render_ms = halves_ms()
                    halves = {"bin_ms": round(bin_ms, 4), "render_ms": round(render_ms, 4)}
                except (ValueError, _lib.SrhError) as exc:
                    print(f"[bench] half-frame probe not available ({exc})", file=sys.stderr)
            if schedule == "frames":
                pipe = make_pipe("frames")
        else:
            pipe = make_pipe(schedule)
        graph_state["on"] = pipe.use_graphs
        graph_state["captured"] = pipe.captured
        n_buf, slabs = n_str, pipe.slabs

        def step(ev=None):
            counter[0] += 1
            pipe.submit(ev)

        def fence():
            pipe.sync()
            torch.cuda.synchronize(device)
    else:
        n_buf = n_str
        frames, slabs = [], []
        for _ in range(n_buf):
            if rank == 0 or frames_par:
                frame = torch.empty((H, 4 * W), dtype=torch.float32, device=device)
                slab = frame[r0:r1]
            else:
                frame = None
                slab = torch.empty((h, 4 * W), dtype=torch.float32, device=device)
            frames.append(frame)
            slabs.append(slab)
        pending = [None] * n_buf

        def step(ev=None):
            b = counter[0] % n_buf
            counter[0] += 1
            if pending[b] is not None:
                with torch.cuda.stream(streams[b]):
                    pending[b].wait()              # this buffer's previous frame has left
                pending[b] = None
            image, depth = views(slabs[b])
            enqueue((b,), streams[b], image, depth, scratch[b], ev)
            if not frames_par:
                with torch.cuda.stream(streams[b]):
                    pending[b] = gather_rows(slabs[b], frames[b], H, dst=0, async_op=True, slabs=cost_parts)

        def fence():
            for b in range(n_buf):
                if pending[b] is not None:
                    pending[b].wait()
                    pending[b] = None
            torch.cuda.synchronize(device)
            dist.barrier()
            torch.cuda.synchronize(device)

    if args.dump_outputs and pipe is None:
        raise SystemExit("--dump-outputs needs the single-process frame pipeline (no process group, no --batch-call on "
                         "with --as-rank)")
    # capture every output slot's graph up front, before any collective is in flight (the single-process pipeline
    # has captured its own)
    if graph_state["on"] and use_dist and not owner:
        if batched:
            for b in range(n_bat):
                for k in range(world):
                    at = 0
                    for j, (a, b_) in enumerate(pieces):
                        enqueue((b, k, j), streams[k % n_str], *views(send[b][k][at:at + (b_ - a)]),
                                scratch[k % n_str], None, rows=(a, b_))
                        at += b_ - a
        else:
            for b in range(n_buf):
                enqueue((b,), streams[b], *views(slabs[b]), scratch[b], None)
        torch.cuda.synchronize(device)
        if os.environ.get("SRH_BENCH_ADDRMAP"):
            # diagnostic: every buffer a replay can touch, and the process's mappings, written out
            # right after capture so that a faulting address reported by the driver can be attributed
            amap = {"scratch": [(t.data_ptr(), t.numel()) for t in scratch],
                    "scene": {k: (t.data_ptr(), t.numel() * t.element_size()) for k, t in buf.tensors.items()}}
            if batched:
                amap["send"] = [(t.data_ptr(), t.numel() * 4) for t in send]
                amap["recv"] = [(t.data_ptr(), t.numel() * 4) for t in recv]
            else:
                amap["slabs"] = [(t.data_ptr(), t.numel() * 4) for t in slabs]
            with open(os.environ["SRH_BENCH_ADDRMAP"], "w") as fh:
                json.dump({k: ([(hex(a), n) for a, n in v] if isinstance(v, list) else
                               {kk: (hex(a), n) for kk, (a, n) in v.items()}) for k, v in amap.items()}, fh, indent=1)
                fh.write("\n--- /proc/self/maps ---\n")
                fh.write(open("/proc/self/maps").read())
                fh.flush()
                os.fsync(fh.fileno())
    # Warm-up: the --warmup steps, then more untimed frames until --warmup-ms of wall time have passed since the first
    # one -- a handful of 0.1 ms frames does not bring the clocks up, and the timed region of a short run would then
    # be measured on a cold GPU.  Every rank runs the same number of extra frames (they contain collectives).
    t_w = time.perf_counter()
    for _ in range(args.warmup):
        step()
    fence()
    warm_steps = args.warmup
    spent = time.perf_counter() - t_w
    if use_dist:
        t = torch.tensor([spent], dtype=torch.float64, device=device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        spent = float(t.item())
    left = args.warmup_ms * 1e-3 - spent
    if left > 0:
        per = max(spent / max(args.warmup, 1), 2e-5) if args.warmup > 0 else 2e-4
        chunk = max(world, 32) // world * world                 # whole batches
        extra = int(min(max(left / per, chunk), 20000)) // chunk * chunk
        done = 0
        while done < extra:
            for _ in range(chunk):
                step()
            done += chunk
            fence()
            if not use_dist and time.perf_counter() - t_w >= args.warmup_ms * 1e-3:
                break                                           # single process: stop on the clock
        warm_steps += done
    warm_ms = 1e3 * (time.perf_counter() - t_w)
    if pipe is not None and args.check:
        pipe.poison()                                           # the check below then proves the timed frames wrote their slabs
    t0 = time.perf_counter()
    for i in range(args.steps):
        step(events[i])
    fence()
    elapsed = time.perf_counter() - t0
    if use_dist:
        t = torch.tensor([elapsed], dtype=torch.float64, device=device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, pipe.slabs[(pipe.count - 1) % pipe.n], W, r0)

    check_note = None
    # A multi-rank schedule (owner-weighted or batched all-to-all) whose frames fail the bit-for-bit check on ANY rank does
    # not end the run: every rank learns of it (one all-reduce), the headline then comes from the metric's literal form
    # below -- equal slabs, one gather per frame to rank 0, checked the same way -- and the line says so.
    collection_failed = False
    if args.check and owner:
        ref = torch.empty((H, 4 * W), dtype=torch.float32, device=device)
        renderer.render_buffers(buf, cam, rows=(0, H), mode=args.mode, out=(*views(ref), None))
        torch.cuda.synchronize(device)
        rendered = warm_steps + args.steps
        got = [recv[b] for b in range(n_bat)
               if batcher.delivered[b] >= 0 and batcher.delivered[b] * world + rank < rendered]
        # the whole frame assembled on this rank, every rank's rows
        bad = any(not torch.equal(t.view(torch.int32), ref.view(torch.int32)) for t in got)
        collection_failed = ranks_agree_failed(bad, rank, device, "an assembled frame differs from the eager full-frame render")
        check_note = f"{len(got)} assembled frame(s) equal the eager full-frame render bit for bit"
        if rank == 0 and not collection_failed:
            print(f"[bench] check ok: {check_note}", file=sys.stderr)
    elif args.check and pipe is not None:
        try:
            n_ok = pipe.verify()
        except RuntimeError as exc:
            raise SystemExit(f"[bench] check FAILED: {exc}")
        check_note = f"{n_ok} output slab(s) of the timed frames equal an eager render bit for bit"
        print(f"[bench] check ok: {check_note}", file=sys.stderr)
    elif args.check and use_dist:
        ref = torch.empty((h, 4 * W), dtype=torch.float32, device=device)
        at = 0
        for a, b_ in pieces:
            renderer.render_buffers(buf, cam, rows=(a, b_), mode=args.mode, out=(*views(ref[at:at + (b_ - a)]), None))
            at += b_ - a
        torch.cuda.synchronize(device)
        if batched:                                    # my own slab inside the frames assembled on this rank
            rendered = warm_steps + args.steps         # frames really rendered (a partial last batch has empty slots)
            got = [recv[b][rank] for b in range(n_bat)
                   if batcher.delivered[b] >= 0 and batcher.delivered[b] * world + rank < rendered]
        else:
            got = [slabs[b] for b in range(min(n_buf, counter[0]))]
        bad = any(not torch.equal(t.view(torch.int32), ref.view(torch.int32)) for t in got)
        collection_failed = ranks_agree_failed(bad, rank, device, "a collected frame differs from the eager render")
        if collection_failed and not (batched and world > 1):
            # this WAS the plain gather to rank 0 (or a one-rank rehearsal): nothing simpler to fall back to
            raise SystemExit("[bench] check FAILED: a collected frame differs from the eager render")
        check_note = f"{len(got)} collected slab(s) equal the eager render bit for bit"
        if rank == 0 and not collection_failed:
            print(f"[bench] check ok: {check_note}", file=sys.stderr)

    # Multi-GPU runs also report the metric's literal form (one gather per frame to rank 0, equal contiguous slabs) and
    # the measured rate of both collections on this node's links, so the first hardware run replaces the link model of
    # DESIGN.md section 5 with data.  Every rank takes part; outside the timed region above.
    literal = link = None
    if use_dist and not frames_par and not args.as_rank and \
            (os.environ.get("SRH_BENCH_BACKEND", "nccl") == "nccl" or os.environ.get("SRH_BENCH_LITERAL")):
        already_literal = not batched
        if args.full:
            link = measure_exchange(device, rank, world, W, H)
        if not already_literal:
            literal = literal_root0_leg(args, buf, cam, device, rank, world, W, H)

    if collection_failed and (literal is None or literal.get("failed")):   # nothing correct to fall back to
        raise SystemExit("[bench] check FAILED: the collected frames differ from the eager render")

    timed = [e for e in events if e is not None and (not args.as_rank or args.batch_call != "on")]
    kernel_ms = float(np.mean([e.elapsed_ms() for e in timed])) if timed else 0.0
    for e in events:
        if e is not None:
            e.close()

    if rank == 0:
        fps = args.steps / elapsed * (world if frames_par else 1)      # every rank delivered `steps` whole frames
        tests = float(M) * W * H
        # algorithmic HBM bytes of one render launch on this rank: primitives read once in the
        # reference's layout (pos 16 + normal 16 + radius 4 + material_idx 4 = 40 B) + rgb and depth written once
        timed_rows = pieces[0][1] - pieces[0][0]           # rows of the launch the event pairs bracket
        alg_bytes = M * 40.0 + timed_rows * W * (12.0 + 4.0)
        ach_gbs = alg_bytes / (kernel_ms * 1e-3) / 1e9 if kernel_ms > 0 else 0.0
        default_workload = (M, W, H, world) == (100_000, 2048, 2048, 1) and args.mode in ("auto", "binned") \
            and not args.as_rank
        pmc = load_pmc() if default_workload else None
        lib_match = "unknown"
        if pmc:
            try:
                import hashlib
                with open(_lib.lib_path(), "rb") as fh:
                    same = hashlib.sha256(fh.read()).hexdigest() == pmc["lib_sha256"]
                lib_match = "the library this run loaded" if same else "NOT the library this run loaded"
            except Exception:                               # noqa: BLE001
                pass
        valu_n = pmc["valu_wave_instr"] if pmc else 0.0
        ginstr_s = valu_n / (kernel_ms * 1e-3) / 1e9 if kernel_ms > 0 else 0.0
        out = {
            "metric": "frames/s + Gray-prim tests/s, 2048² × 100k disk splats, 1/2/4/8 MI355X",
            "value": fps, "unit": "frames/s", "gtests_per_s": fps * tests / 1e9,
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": 1e3 * elapsed / args.steps, "higher_is_better": True,
            "scaling": "weak" if frames_par else "strong",
            "vs_baseline": None,
            "dtype": "f64" if args.mode == "exact" else "f32 reject + f64 confirm",
            "data": "synthetic",
            "config": {"workload": "BASELINE configs[4]: 100k synthetic disk splats, 2048x2048, forward render, "
                                   "framebuffer row-tiled across ranks + 1 gather",
                       "prims": M, "width": W, "height": H, "lights": 4, "mode": args.mode,
                       "frames_in_flight": n_str, "schedule": schedule if pipe is not None else "frames",
                       "schedule_probe": halves,
                       "launch": f"hipGraph replay ({graph_state['captured']} graphs)"
                                 if graph_state["on"] and graph_state["captured"] else "eager",
                       "warmup_steps_run": warm_steps, "warmup_ms_run": warm_ms,
                       "check": check_note if args.check else "off",
                       "parallelism": (f"frames/{world}" if frames_par else f"rows/{world}") if not args.as_rank
                                      else f"rehearsal of rank {args.as_rank}",
                       "launches": ("one srh_render_views call per batch of frames"
                                    if batched and args.batch_call != "off" and (not owner or cost_parts is not None)
                                    else "per frame"),
                       "rows_per_rank": (f"work-balanced contiguous slabs (bin lengths of a probe frame): "
                                         f"{[b_ - a for a, b_ in cost_parts]} rows" if cost_parts is not None else
                                         f"owner-weighted: the rank that assembles a frame renders {max(recv_rows)} of "
                                         f"its {H} rows, the others {min(recv_rows)} each" if owner else
                                         "two half-slabs, g and P+g of 2P" if balanced else "one contiguous slab"),
                       "collection": "none" if (not use_dist or frames_par) else
                                     (f"all-to-all per {world} frames{' (unequal splits)' if owner else ''}, frame k on rank k" if batched
                                      else "gather to rank 0 per frame")},
            "roofline": {"bound": "hbm", "achieved": ach_gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": ach_gbs / HBM_PEAK_GBS,
                         "traffic": pmc["traffic_bytes"] if pmc else None,
                         "traffic_source": (f"{pmc['file']}: rocprofv3 --pmc WRITE_SIZE + 2 x FETCH_SIZE (separate "
                                            f"passes, per launch), taken at commit {pmc['commit']}, libsrh.so sha256 "
                                            f"{str(pmc['lib_sha256'])[:12]} ({lib_match}); not re-measured by this run")
                         if pmc else None,
                         "kernel": "render kernel of rank 0", "kernel_ms": kernel_ms,
                         "algorithmic_bytes": alg_bytes,
                         # `kernel_ms` is one launch's duration WHILE `concurrent_launches` frames share the GPU (their
                         # render kernels overlap); per unit of job time the kernel moves alg_bytes every ms_per_step
                         "concurrent_launches": (args.render_streams if (pipe is not None and schedule == "stages") else n_str),
                         "achieved_per_job_time": alg_bytes / (elapsed / args.steps) / 1e9,
                         "note": "the kernel is bound by vector-instruction issue, not by HBM; see valu_issue"},
            # SURVEY 8d's figure: algorithmic flops of ALL (pixel, primitive) pairs per second against the fp32 vector
            # peak.  All-pairs evaluation tops out at frac = 1 (about 22 frames/s); the binned kernel proves most pairs
            # cannot matter and never evaluates them, hence a value far above 1.
            "valu_algorithmic": {"achieved": fps * tests * FLOP_PER_DISK_TEST / 1e12, "peak": VALU_F32_PEAK_TFLOPS,
                                 "unit": "TFLOP/s (algorithmic, all pairs)",
                                 "frac": fps * tests * FLOP_PER_DISK_TEST / 1e12 / VALU_F32_PEAK_TFLOPS,
                                 "flop_per_test": FLOP_PER_DISK_TEST},
            "valu_issue": ({"achieved": ginstr_s, "peak": VALU_PEAK_GINSTR_S, "unit": "G wave-instr/s",
                            "frac": ginstr_s / VALU_PEAK_GINSTR_S,
                            "frac_per_job_time": valu_n / (elapsed / args.steps) / 1e9 / VALU_PEAK_GINSTR_S,
                            "wave_instr_per_launch": valu_n,
                            "source": f"SQ_INSTS_VALU from {pmc['file']} (commit {pmc['commit']}) over the live "
                                      "kernel time; peak = one wave-instruction per SIMD per 4 cycles "
                                      "(profiles/r02_ubench_issue.txt); peak_mix_weighted prices the kernel's own mix"}
                           if pmc else None),
        }
        if out["valu_issue"] is not None:
            # the same achieved rate against a ceiling weighted by the kernel's instruction mix: the 2.5-cycle classes
            # (add / sub / mul_f32, logic, shifts, integer add, mov) are a third of the sweep (tools/valu_mix.py)
            try:
                with open(MIX_FILE) as fh:
                    peak_mix = float(json.load(fh)["launch"]["peak_ginstr_s_mix_weighted"])
                out["valu_issue"].update(peak_mix_weighted=peak_mix, frac_mix_weighted=ginstr_s / peak_mix,
                                         frac_per_job_time_mix_weighted=valu_n / (elapsed / args.steps) / 1e9 / peak_mix,
                                         mix_source=os.path.relpath(MIX_FILE, REPO))
            except Exception:                                   # noqa: BLE001 -- no file, no figure
                pass
        # the pairs the kernel really tests (bin lengths of one frame, read back outside the timed region) beside the
        # algorithmic primitives x pixels of `gtests_per_s` -- SURVEY 8 f2
        if args.full and args.mode in ("auto", "binned") and not args.as_rank and world == 1:
            try:
                st = renderer.bin_statistics(buf, cam)
                out["executed_pair_tests"] = {"per_frame": st["executed_pair_tests"],
                                              "algorithmic_per_frame": st["algorithmic_pair_tests"],
                                              "fraction": st["executed_pair_tests"] / st["algorithmic_pair_tests"],
                                              "gtests_per_s_executed": fps * st["executed_pair_tests"] / 1e9,
                                              "tile_list_entries": st["executed_pair_tests"] // 256,
                                              "what": "(tile, primitive) list entries x 256 pixels: the pairs that go through "
                                                      "the fp32 reject test; every other pair was ruled out by the binning"}
            except Exception as exc:                            # noqa: BLE001
                print(f"[bench] executed_pair_tests not available ({exc!r})", file=sys.stderr)
        if literal is not None:
            out["literal_root0"] = literal
        if literal is not None and not literal.get("failed") and (collection_failed or literal["value"] > out["value"]):
            # Two schedules were run and checked under the same rules (warm-up, exactly --steps frames, barrier on both
            # sides, max over ranks): the rotating-root default above and the metric's literal form.  The headline is the
            # faster CORRECT one -- the default has never met real xGMI links, and a schedule whose frames failed the
            # bit-for-bit check on any rank is not a result at all.  The other one stays visible under its own key.
            out["other_schedule"] = {"value": out["value"], "ms_per_step": out["ms_per_step"],
                                     "collection": out["config"]["collection"],
                                     "rows_per_rank": out["config"]["rows_per_rank"],
                                     "status": ("bit-for-bit check FAILED on at least one rank; not a result"
                                                if collection_failed else "checked; slower than the literal form in this run")}
            out["value"], out["ms_per_step"] = literal["value"], literal["ms_per_step"]
            out["gtests_per_s"] = literal["value"] * tests / 1e9
            out["config"].update(collection=literal["collection"], rows_per_rank=literal["rows_per_rank"],
                                 launch=literal["launch"], frames_in_flight=literal["frames_in_flight"],
                                 launches="per frame", check=literal["check"])
            for key in ("roofline", "valu_issue"):     # their kernel time was taken inside the other schedule
                if out.get(key):
                    out[key]["note"] = "kernel time measured inside the schedule reported under other_schedule"
        if use_dist and literal is not None:
            out["config"]["schedule_choice"] = ("two schedules timed and checked in this run; the faster correct one is "
                                                "`value`" if args.check else
                                                "two schedules timed in this run (not checked); the faster one is `value`")
        if link is not None:
            out["links_measured"] = link
        if args.full and world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(scene, M, W, H, args.cpu_pixels)
        if collection_failed:
            # a schedule that RAN failed its check: the numbers above are the literal form's (which passed), but a
            # correctness failure of the production collection path must not read as a passing benchmark
            out["check_failed"] = True
        print(json.dumps(out), flush=True)
    if use_dist:
        dist.barrier()
        dist.destroy_process_group()
    if collection_failed and not args.allow_fallback:     # agreed on by every rank (ranks_agree_failed)
        raise SystemExit(3)


if __name__ == "__main__":
    main()
