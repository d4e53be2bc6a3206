#!/usr/bin/env python3
"""Headline benchmark (BASELINE.json): images/sec of the DensePose hot path on R_50_FPN_s1x, 800x1333 frames,
batch 8 per GPU, bf16 operands / fp32 accumulate, detections pinned to R = 8 per image.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR]

N > 1: one rank per GPU. Under torch.distributed.run (RANK / WORLD_SIZE in the environment) this process IS a rank; run
bare (`python bench.py --gpus 8`) it starts the N ranks itself as child processes - before anything here touches the
GPU - and exits with the first failing rank's code.

A "step" = one pass of the whole path (device resize -> backbone -> RPN -> box head -> DensePose head -> IUV maps)
over one batch of synthetic frames that are already resident in HBM. Prints ONE JSON line on rank 0.
"""
import argparse
import glob
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_BF16_DENSE = 2.5e15   # MI355X dense bf16 MFMA (MI355X_MICROARCH.md: "~2.5 PF dense")
PEAK_F32_MATRIX = 157.3e12
PEAK_HBM = 8.0e12          # HBM3E, bytes/s (MI355X_MICROARCH.md: 8 TB/s spec, 6.3 TB/s measured with a float4 copy)
HBM_PEAK = 8.0e12


def make_frames(n, start, hw, device):
    h, w = hw
    return [torch.from_numpy(np.random.default_rng(1234 + start + i).integers(0, 256, (h, w, 3), dtype=np.uint8)).to(device)
            for i in range(n)]


DUMP_BUDGET_BYTES = 60 << 20   # --dump-outputs writes at most this much array data (the limit is 64 MB with the .npy headers)


def dump_outputs(out, directory, budget_bytes=DUMP_BUDGET_BYTES):
    """--dump-outputs DIR: the results one timed step returned to its caller, one `frame<i>_<key>.npy` per frame and key.
    Floating outputs are written as float32, integer ones as float64 (exact). When the whole would exceed `budget_bytes`,
    every array of more than 2**16 elements (the IUV maps) is replaced by the same fraction of its elements, taken in
    ascending flat-index order at the positions np.random.default_rng(0).choice(size, count, replace=False) selects: the
    sample depends only on the array's shape, so two builds that return equal shapes are compared element for element."""
    arrays = {}
    for i, res in enumerate(out):
        for k, v in res.items():
            a = v.detach().cpu()
            a = a.double() if not a.is_floating_point() else a.float()
            arrays["frame%d_%s" % (i, k)] = a.numpy()
    big = {k for k, a in arrays.items() if a.size > 1 << 16}
    small_bytes = sum(a.nbytes for k, a in arrays.items() if k not in big)
    big_bytes = sum(arrays[k].nbytes for k in big)
    frac = 1.0 if small_bytes + big_bytes <= budget_bytes else max(0.0, budget_bytes - small_bytes) / big_bytes
    os.makedirs(directory, exist_ok=True)
    for k, a in arrays.items():
        if k in big and frac < 1.0:
            idx = np.sort(np.random.default_rng(0).choice(a.size, int(a.size * frac), replace=False))
            a = a.reshape(-1)[idx]
        np.save(os.path.join(directory, k + ".npy"), a)


def cpu_baseline(cfg, state, hw, budget_s):
    """The oracle (a CPU port of the reference path, oracle/ref_cpu.py) timed on this box's host cores on a bounded
    sample of the same workload (same weights, same frames, same R): 3 warm-up frames, then 10 timed ones,
    fewer only if the box is so slow that 10 would not fit the budget."""
    from oracle.ref_cpu import OracleModel
    # torch's CPU convolutions stop scaling (and then collapse) beyond a few dozen threads on this class of host: the whole path at
    # 8 / 16 / 32 / 64 threads of the 256-CPU GPU box runs at 0.73 / 0.88 / 0.67 / 0.33 images/s, nproc does not finish a frame in a
    # minute (tools/cpu_threads.py, profiles/r5_cpu_threads.txt) - the baseline is timed at the thread count that serves it best
    cores = min(os.cpu_count() or 1, 16)
    torch.set_num_threads(cores)
    os.environ["OMP_NUM_THREADS"] = str(cores)
    model = OracleModel(cfg, state)
    frames = [torch.from_numpy(np.random.default_rng(1234 + i).integers(0, 256, (hw[0], hw[1], 3), dtype=np.uint8)) for i in range(8)]
    warm = []
    for i in range(3):
        t0 = time.time()
        model(frames[i])
        warm.append(time.time() - t0)
    n_timed = max(3, min(10, int(budget_s / max(min(warm), 1e-3))))
    times = []
    for i in range(n_timed):
        t0 = time.time()
        model(frames[i % 8])
        times.append(time.time() - t0)
    return {"value": round(len(times) / sum(times), 4), "unit": "images/s", "cores": cores, "kind": "port",
            "sample": "%d frame(s) %dx%d %s fp32 after 3 warm-up frames, oracle/ref_cpu.py (torch %s CPU + C roi_align/nms), p50 %.0f ms/img"
                      % (len(times), hw[0], hw[1], cfg.name if hasattr(cfg, "name") else "R_50_FPN_s1x", torch.__version__, 1e3 * float(np.median(times)))}


def accuracy_vs_golden(pred, dtype):
    """The throughput dtype against the reference's fp32 golden of the SAME workload (tests/golden/full_r50_s1x_800x1333.npz:
    frame 0 of this benchmark, same weights, R = 8; recorded from the imported reference by oracle/make_goldens.py):
    how many reference detections are found (box within 1 px, score within 0.02) and the largest IUV deviation on them."""
    path = os.path.join(ROOT, "tests", "golden", "full_r50_s1x_800x1333.npz")
    if not os.path.exists(path):
        return None
    z = np.load(path)
    meta = json.loads(bytes(z["meta"]).decode())
    img = np.random.default_rng(meta["image_seed"]).integers(0, 256, tuple(meta["image_hw"]) + (3,), dtype=np.uint8)
    out = pred(torch.from_numpy(img).to(pred.device))
    torch.cuda.synchronize()
    s = meta["iuv_stride"]
    boxes, scores = out["pred_boxes"].float().cpu().numpy(), out["scores"].float().cpu().numpy()
    rb, rs = z["out/pred_boxes"], z["out/scores"]
    matched, iuv_err, box_err, score_err = 0, 0.0, 0.0, 0.0
    pairs = []
    used = np.zeros(len(boxes), dtype=bool)
    for i in range(len(rb)):
        if not len(boxes):
            break
        d = np.abs(boxes - rb[i]).max(axis=1)
        d[used] = np.inf
        j = int(d.argmin())
        if d[j] <= 1.0 and abs(float(scores[j]) - float(rs[i])) <= 0.02:
            used[j] = True
            matched += 1
            pairs.append((i, j))
            box_err, score_err = max(box_err, float(d[j])), max(score_err, abs(float(scores[j]) - float(rs[i])))
            for k in ("pred_densepose_coarse_segm", "pred_densepose_fine_segm", "pred_densepose_u", "pred_densepose_v"):
                iuv_err = max(iuv_err, float(np.abs(out[k][j].float().cpu().numpy()[:, ::s, ::s] - z["out/" + k][i]).max()))
    # part-index agreement (the north star's second parity clause): the visualiser's labels (visualizer.py:10-30: argmax of the
    # fine segmentation where the coarse one says foreground) computed from THIS run's IUV maps of every matched detection, on
    # the reference's box of that detection (same crop size as the golden's labels, recorded at full map resolution), against
    # the golden's labels: fraction of equal pixels over all matched detections, and over the reference's foreground pixels
    labels = None
    if pairs:
        from densepose_torchscript_amd.visualizer import extract_iuv
        js = torch.tensor([j for _, j in pairs], device=out["pred_boxes"].device)
        sub = {k: out[k][js].float().contiguous() for k in ("pred_densepose_coarse_segm", "pred_densepose_fine_segm", "pred_densepose_u", "pred_densepose_v")}
        sub["pred_boxes"] = torch.from_numpy(np.stack([rb[i] for i, _ in pairs])).to(js.device)
        res, _ = extract_iuv(sub)
        torch.cuda.synchronize()
        eq = tot = eq_fg = tot_fg = 0
        for (i, _), r in zip(pairs, res):
            want, got = z["vis/labels_%d" % i], r["labels"].cpu().numpy()
            if want.shape != got.shape:
                continue
            eq, tot = eq + int((want == got).sum()), tot + want.size
            fg = want > 0
            eq_fg, tot_fg = eq_fg + int((want[fg] == got[fg]).sum()), tot_fg + int(fg.sum())
        if tot:
            labels = {"label_agreement": round(eq / tot, 5), "label_agreement_foreground": round(eq_fg / max(tot_fg, 1), 5),
                      "label_pixels": tot, "label_note": "vis/labels_* of the golden vs dp_iuv_extract on this run's maps, matched detections, full resolution"}
    # the reference's OWN run in this dtype on the same frame (tests/golden/..__bf16.npz: predictor.bfloat16() on the CPU, run.py:20-29 /
    # export.py:36-37) and this run, both against the fp32 golden under ONE definition (tests/yardstick.py: a detection counts as found
    # when the nearest box is within 1.5 px; IUV deviation relative to the map's largest fp32 value; labels on the fp32 run's boxes)
    yard = None
    lp = os.path.join(ROOT, "tests", "golden", "full_r50_s1x_800x1333__%s.npz" % {"bf16": "bf16", "fp16": "half"}.get(dtype, "none"))
    if os.path.exists(lp):
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        try:
            from yardstick import engine_distance, lowp_distance_from_fixtures
            from densepose_torchscript_amd.visualizer import extract_iuv as _gpu_extract

            def _extract(sub):      # the GPU visualiser extract (dp_iuv_extract) in the CPU oracle's calling convention
                res, _ = _gpu_extract({k: v.to(pred.device) for k, v in sub.items()})
                return [(r["labels"].cpu(), None) for r in res]
            cpu_out = {k: v.float().cpu() if v.is_floating_point() else v.cpu() for k, v in out.items()}
            rnd = lambda d: {k: (round(v, 5) if isinstance(v, float) else v) for k, v in d.items()}   # noqa: E731
            yard = {"definition": "tests/yardstick.py", "this_run": rnd(engine_distance(cpu_out, z, s, _extract)),
                    "reference_in_this_dtype": rnd(lowp_distance_from_fixtures(z, np.load(lp))),
                    "reference_fixture": os.path.relpath(lp, ROOT),
                    "note": "seeded random weights: detections sit next to the score threshold, so both runs lose some of the fp32 run's "
                            "detections; a real checkpoint cannot be evaluated here (no .pkl on either box)"}
        finally:
            sys.path.pop(0)
    return {"reference": "tests/golden/full_r50_s1x_800x1333.npz (fp32, recorded from the imported reference)", "dtype": dtype,
            **(labels or {}), **({"yardstick": yard} if yard else {}),
            "ref_detections": int(len(rb)), "detections": int(len(boxes)), "box_match_rate": round(matched / max(len(rb), 1), 3),
            "max_abs_box_err_px": round(box_err, 4), "max_abs_score_err": round(score_err, 5),
            "max_abs_iuv_err_on_matched": round(iuv_err, 4), "iuv_samples": "every %dth pixel of the 112x112 maps" % s}


def r_sensitivity(args, state, frames, device):
    """images/s of the same workload with the detection count pinned to R = 0 and to R = 100 per image (the
    DensePose head costs 28.7 GFLOP per detection, so the result is linear in R; the headline runs at R = 8)."""
    from densepose_torchscript_amd import get_config
    from densepose_torchscript_amd.options import EngineOptions
    from densepose_torchscript_amd.predictor import DensePosePredictor
    out = {}
    for label, opts in (("R0", ["TEST.DETECTIONS_PER_IMAGE", 8, "MODEL.ROI_HEADS.SCORE_THRESH_TEST", 2.0]),
                        ("R100", ["TEST.DETECTIONS_PER_IMAGE", 100, "MODEL.ROI_HEADS.SCORE_THRESH_TEST", 0.0])):
        cfg = get_config(args.config, opts)
        p = DensePosePredictor(cfg, state, dtype=args.dtype, device=device, resize="device", use_graphs=not args.no_graphs, options=EngineOptions.from_env())
        p.pipeline_depth = args.pipeline
        for _ in range(4):
            res = p.predict_batch(frames)
        p.join()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = 6
        for _ in range(n):
            res = p.predict_batch(frames)
        p.join()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        out[label] = {"images_per_s": round(n * len(frames) / dt, 1), "measured_R": [int(o["scores"].shape[0]) for o in res]}
        del p
        torch.cuda.empty_cache()
    return out


def multi_gpu_record(values, world, device, extra=None):
    """`multi_gpu` of the JSON line: what every rank measured for itself, as MIN / MAX / per-rank lists (the driver computes scaling
    efficiency from `value`; this says WHERE a shortfall comes from - the host feed path or the GPUs)."""
    from densepose_torchscript_amd.parallel import rank_stats
    import torch.distributed as dist
    stats = rank_stats(values, device)
    info = None
    if extra is not None:      # per-rank strings (device name, CPU share): one all_gather_object
        info = [None] * (dist.get_world_size() if dist.is_initialized() else 1)
        if dist.is_initialized() and dist.get_world_size() > 1:
            dist.all_gather_object(info, extra)
        else:
            info = [extra]
    return {"ranks_in_process_group": dist.get_world_size() if dist.is_initialized() else 1, "world": world,
            "backend": dist.get_backend() if dist.is_initialized() else None, **stats, **({"per_rank_info": info} if info else {}),
            "note": "sustained / host_frames: every rank runs the loop at the same time (frames resident in HBM / starting in pageable host "
                    "memory on every rank at once); weight_broadcast: the one RCCL broadcast of the packed weights from rank 0"}


def rocprof_average_us(kernel_cls, args):
    """(average launch of `kernel_cls` in microseconds, file) from the newest committed rocprofv3 --stats summary of the serialized configuration
    (profiles/r*_kernel_stats_streams1_nographs.csv), or None - headline workload only. `kernel_cls` is the engine's class label, e.g.
    conv3x3_rows2_kernel<512>; the CSV has the demangled template instance, e.g. conv3x3_rows2_kernel<unsigned short, 512>(...)."""
    import csv
    import re
    if not (args.dtype == "bf16" and args.config == "densepose_rcnn_R_50_FPN_s1x" and args.batch == 8):
        return None
    m = re.match(r"(\w+)<(.*)>$", kernel_cls)
    base, targs = (m.group(1), [a.strip() for a in m.group(2).split(",")]) if m else (kernel_cls, [])
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_kernel_stats_streams1_nographs.csv")), reverse=True):
        for row in csv.DictReader(open(path)):
            name = row.get("Name", "")
            mm = re.search(r"::%s<([^>]*)>\(" % re.escape(base), name)
            if not mm:
                continue
            have = [a.strip() for a in mm.group(1).split(",")]
            if have[:1] != ["unsigned short"]:
                continue
            if all(a in have for a in targs if a.isdigit()):
                return round(float(row["AverageNs"]) / 1e3, 2), "profiles/" + os.path.basename(path)
    return None


def spawn_selftest():
    """`--spawn-selftest`: what a rank does up to the first collective, without a GPU (gloo) - exercised by the CPU tests
    to cover the self-launch path of `bench.py --gpus N`."""
    import torch.distributed as dist
    from densepose_torchscript_amd import parallel
    rank, local_rank, world = parallel.init_distributed(backend="gloo")
    t = torch.tensor([1.0 + rank], dtype=torch.float64)
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dist.barrier()
    # the multi-rank part of the benchmark record, with stand-in numbers: same keys, same collective (parallel.rank_stats)
    cpus = parallel.pin_rank_to_cpus()
    multi = multi_gpu_record({"sustained_images_per_s": 100.0 + rank, "host_frames_images_per_s": 90.0 - rank,
                              "weight_broadcast_s": 0.01 * (rank + 1), "weight_broadcast_bytes": 1.0e6}, world, None,
                             extra={"rank": rank, "device": "selftest", "local_rank": local_rank, "cpus": (len(cpus) if cpus else None),
                                    "first_cpu": (cpus[0] if cpus else None), "host_gather_workers": parallel.host_workers(4)})
    if rank == 0:
        print(json.dumps({"selftest": "spawn", "world": world, "max_over_ranks": float(t.item()), "multi_gpu": multi}), flush=True)
    if world > 1:
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8, help="frames per GPU per step")
    ap.add_argument("--config", default="densepose_rcnn_R_50_FPN_s1x")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16", "fp32"])
    ap.add_argument("--dets", type=int, default=8, help="detections per image (R), pinned via TEST.DETECTIONS_PER_IMAGE")
    ap.add_argument("--height", type=int, default=800)
    ap.add_argument("--width", type=int, default=1333)
    ap.add_argument("--streams", type=int, default=1, help="sub-batches of a step run concurrently on this many HIP streams")
    ap.add_argument("--pipeline", type=int, default=2, help="stream lanes consecutive batches alternate between (1 = off)")
    ap.add_argument("--no-overlap", action="store_true", help="decoder in line instead of on a side stream")
    ap.add_argument("--no-fork", action="store_true", help="independent per-level layers in line instead of on forked streams")
    ap.add_argument("--no-graphs", action="store_true", help="launch every kernel eagerly instead of replaying HIP graphs")
    ap.add_argument("--no-roofline", action="store_true", help="skip the event-instrumented roofline pass (profiling runs)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-budget-s", type=float, default=25.0)
    ap.add_argument("--no-extras", action="store_true", help="skip the accuracy / R-sensitivity / single-frame latency extras")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step returned as DIR/<name>.npy (rank 0's frames; see dump_outputs; "
                         "bench_outputs/ is git-ignored)")
    ap.add_argument("--spawn-selftest", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    # ---- self-launch: `python bench.py --gpus N` without a launcher starts its own N ranks (fresh child processes, started
    # before this process has made any GPU call; a process that initialised the GPU is never re-executed)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        from densepose_torchscript_amd.parallel import launch_local_ranks
        sys.exit(launch_local_ranks([os.path.abspath(__file__)] + sys.argv[1:], args.gpus))
    if args.spawn_selftest:
        return spawn_selftest()

    from densepose_torchscript_amd import get_config, make_synthetic_state
    from densepose_torchscript_amd import parallel
    from densepose_torchscript_amd.options import EngineOptions
    from densepose_torchscript_amd.predictor import DensePosePredictor
    from densepose_torchscript_amd.weights import param_shapes
    import torch.distributed as dist

    # a rank's host threads stay on its share of the CPUs (in-process sched_setaffinity, BEFORE the process group / the GPU context
    # spawn their helper threads, which inherit the mask)
    rank_cpus = parallel.pin_rank_to_cpus()
    rank, local_rank, world = parallel.init_distributed()
    if world != args.gpus:
        raise SystemExit("bench.py: WORLD_SIZE=%d but --gpus %d" % (world, args.gpus))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the product path has no CPU fallback")
    torch.cuda.set_device(local_rank)
    device = "cuda:%d" % local_rank
    dist_info = None
    if world > 1:
        # first thing an N-rank run says (stderr; stdout stays the one JSON line): what it runs on
        try:
            rccl = ".".join(str(v) for v in torch.cuda.nccl.version())
        except Exception as e:      # noqa: BLE001
            rccl = "unknown (%s)" % type(e).__name__
        dist_info = {"backend": dist.get_backend(), "rccl_version": rccl, "ranks_in_process_group": dist.get_world_size(),
                     "HSA_ENABLE_IPC_MODE_LEGACY": os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY")}
        if rank == 0:
            print("bench.py: %d ranks in the process group, backend %s (RCCL %s), HSA_ENABLE_IPC_MODE_LEGACY=%s"
                  % (dist_info["ranks_in_process_group"], dist_info["backend"], rccl, dist_info["HSA_ENABLE_IPC_MODE_LEGACY"]), file=sys.stderr, flush=True)

    cfg = get_config(args.config, ["TEST.DETECTIONS_PER_IMAGE", args.dets])
    # weights: generated on rank 0 only, then ONE coalesced RCCL broadcast of the packed device tensors (xGMI)
    if rank == 0:
        state = make_synthetic_state(cfg, 0)
    else:
        state = {k: np.zeros(s, dtype=np.float32) for k, s in param_shapes(cfg).items()}
        for k in state:
            if k.endswith("running_var"):
                state[k] += 1.0
    pred = DensePosePredictor(cfg, state, dtype=args.dtype, device=device, resize="device", num_streams=args.streams,
                              use_graphs=not args.no_graphs, options=EngineOptions.from_env())
    bcast_s, bcast_bytes = 0.0, 0
    if world > 1:
        tensors = pred.engine.model.parameter_tensors()
        bcast_bytes = sum(t.numel() * t.element_size() for t in tensors)
        torch.cuda.synchronize()
        dist.barrier()
        t0 = time.perf_counter()
        parallel.broadcast_tensors(tensors, src=0)
        torch.cuda.synchronize()
        bcast_s = time.perf_counter() - t0
    eng = pred.engine
    # `--streams 1 --no-graphs` is the fully serialized configuration (one kernel at a time on the chip) that profiles/ and
    # the roofline pass use; otherwise the decoder also runs beside the RPN / box branch on a side stream
    overlap = not (args.streams == 1 and args.no_graphs) and not args.no_overlap
    eng.overlap_decoder = overlap
    eng.fork_levels = eng.fork_levels if (overlap and not args.no_fork) else 0
    hw = (args.height, args.width)
    frames = make_frames(args.batch, rank * args.batch, hw, device)  # weak scaling: every rank owns `batch` frames
    torch.cuda.synchronize()

    def step():
        return pred.predict_batch(frames)

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    # Timed region: consecutive batches alternate between `--pipeline` stream lanes, so the DensePose-head phase of batch i
    # (launched once the host has read batch i's detection counts) runs beside the backbone / RPN phase of batch i+1.
    # Every batch is complete when the closing device synchronize returns; nothing is skipped or carried over.
    pipelined = not (args.streams == 1 and args.no_graphs)
    pred.pipeline_depth = args.pipeline if pipelined else 1
    for _ in range(max(args.warmup, 2 * pred.pipeline_depth)):   # at least one capture + one replay per lane
        out = step()
    barrier()
    t_begin = time.perf_counter()
    for _ in range(args.steps):
        out = step()
    pred.join()
    barrier()
    elapsed = time.perf_counter() - t_begin
    if args.dump_outputs and rank == 0:
        dump_outputs(out, args.dump_outputs)   # before any later step reuses the buffers the last timed step returned
    # the same loop held for >= 3 s (the K-step region above is ~0.1 s at the default K: too short to say anything about the
    # clock the chip sustains) and, beside it, the same workload with the frames starting in PAGEABLE HOST memory like the
    # reference's run.py:34-36 hands them over (pinned ring + one H2D per batch on a copy stream, predictor._HostFrameRing)
    sustained = host_rate = None
    if not args.no_extras:
        def timed_loop(fr, seconds):
            for _ in range(2 * pred.pipeline_depth):
                pred.predict_batch(fr)
            pred.join()
            torch.cuda.synchronize()
            n, t0 = 0, time.perf_counter()
            while True:
                for _ in range(10):
                    pred.predict_batch(fr)
                n += 10
                if time.perf_counter() - t0 >= seconds:
                    break
            pred.join()
            torch.cuda.synchronize()
            return n * len(fr) / (time.perf_counter() - t0), n
        barrier()                      # N > 1: every rank runs each loop at the same time (per-rank rates: `multi_gpu` below)
        rate, n = timed_loop(frames, 3.0)
        sustained = {"images_per_s": round(rate, 1), "steps": n, "seconds": 3.0}
        host_frames = [f.cpu() for f in frames]
        barrier()
        rate, n = timed_loop(host_frames, 2.0)
        host_rate = {"images_per_s": round(rate, 1), "steps": n,
                     "note": "frames start in pageable host memory each step (3.2 MB each): gathered into a pinned ring slot, "
                             "one H2D per batch on a copy stream"}
    multi = None
    if world > 1:
        multi = multi_gpu_record({"sustained_images_per_s": sustained["images_per_s"] if sustained else 0.0,
                                  "host_frames_images_per_s": host_rate["images_per_s"] if host_rate else 0.0,
                                  "weight_broadcast_s": bcast_s, "weight_broadcast_bytes": float(bcast_bytes)}, world, device,
                                 extra={"rank": rank, "device": torch.cuda.get_device_name(local_rank), "local_rank": local_rank,
                                        "cpus": (len(rank_cpus) if rank_cpus else None), "first_cpu": (rank_cpus[0] if rank_cpus else None),
                                        "host_gather_workers": parallel.host_workers(4)})
    pred.pipeline_depth = 1   # the latency loop and the roofline pass below run batch after batch on one stream
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device=device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    dets = [int(o["scores"].shape[0]) for o in out]
    # p50 latency of one batch (synchronised per step), reported per image
    step_times = []
    for _ in range(max(5, args.steps)):
        t0 = time.perf_counter()
        step()
        torch.cuda.synchronize()
        step_times.append(time.perf_counter() - t0)
    flops_step = eng.flops_last
    # single-frame latency (batch 1, synchronised per call): the number a one-image-at-a-time caller like the reference's
    # run.py sees; the batch p50 above divided by the batch size is a throughput-style per-image figure, not this
    single_times = []
    if not args.no_extras:
        for i in range(13):
            t0 = time.perf_counter()
            pred(frames[i % len(frames)])
            torch.cuda.synchronize()
            if i >= 3:
                single_times.append(time.perf_counter() - t0)

    # ---- roofline of the dominant kernel: K further steps of the same workload, every conv launch bracketed by HIP events
    # on the stream it is launched on. This pass is fully serialized - one stream, no graph replay, no side stream, no
    # pipeline lane - so each kernel has the chip to itself and the event delta is its own duration (in the timed region the
    # decoder and the next batch share the chip with the launch being timed, which inflates per-launch durations).
    # profiles/ holds the rocprofv3 summary of the same serialized configuration (`--streams 1 --no-graphs`), whose
    # per-kernel averages must agree with these.
    if args.no_roofline:
        if rank == 0:
            print(json.dumps({"value": round(args.batch * world * args.steps / elapsed, 3), "ms_per_step": round(1e3 * elapsed / args.steps, 3)}), flush=True)
        return
    from densepose_torchscript_amd.trace import StageTrace
    pred.num_streams, eng.use_graphs, eng.overlap_decoder = 1, False, False
    for _ in range(2):
        step()
    torch.cuda.synchronize()
    # two passes of K steps: per-launch event pairs first (the kernel classes), then stage events only - an event pair around every
    # launch costs a few microseconds of idle chip per launch, which would otherwise be booked on the stages (50 launches in the trunk)
    # (rounds 1 - 4 took both from one pass: that pass's stage times are kept beside the new ones, `with_per_launch_events`)
    eng.prof = []
    eng.trace = StageTrace(device, roctx=False)
    t_ser = time.perf_counter()
    for _ in range(args.steps):
        step()
    torch.cuda.synchronize()
    t_ser = (time.perf_counter() - t_ser) / args.steps
    prof, eng.prof = eng.prof, None
    stages_instr = eng.trace.summary()
    eng.trace = StageTrace(device, roctx=False)
    t_stage = time.perf_counter()
    for _ in range(args.steps):
        step()
    torch.cuda.synchronize()
    t_stage = (time.perf_counter() - t_stage) / args.steps
    stages = eng.trace.summary()
    eng.trace = None
    eng.prof = prof
    agg = {}
    for cls, flops, e0, e1, name, nbytes in eng.prof:
        a = agg.setdefault(cls, [0, 0.0, 0, 0])
        a[0] += flops
        a[1] += e0.elapsed_time(e1) * 1e-3
        a[2] += 1
        a[3] += nbytes
    eng.prof = None
    pred.num_streams, eng.use_graphs, eng.overlap_decoder = args.streams, not args.no_graphs, overlap
    dom = max(agg, key=lambda c: agg[c][1])
    dflops, dsec, dcalls = agg[dom][:3]
    peak = PEAK_F32_MATRIX if args.dtype == "fp32" else PEAK_BF16_DENSE  # fp16 and bf16 MFMA share the dense peak
    traffic = None
    # newest committed PMC summary that has this kernel
    for tname in sorted((os.path.basename(f) for f in glob.glob(os.path.join(ROOT, "profiles", "r*_hbm_traffic.json"))), reverse=True):
        tpath = os.path.join(ROOT, "profiles", tname)
        if traffic is None and os.path.exists(tpath) and args.dtype == "bf16" and args.config == "densepose_rcnn_R_50_FPN_s1x" and args.batch == 8:
            ks = json.load(open(tpath))["kernels"]
            k = ks.get(dom + "[bf16]") or ks.get(dom)      # (tools/pmc_summary.py tags the multi-dtype template families only)
            if k:
                traffic = {"hbm_bytes_per_launch": k["hbm_bytes_per_launch"], "measured_in_this_run": False,
                           "source": "from committed profile: profiles/%s (rocprofv3 --pmc FETCH_SIZE x2 + WRITE_SIZE, separate passes)" % tname}
    roofline = {"bound": "mfma", "kernel": dom, "achieved": round(dflops / dsec / 1e12, 2), "peak": peak / 1e12, "unit": "TFLOP/s",
                "frac": round(dflops / dsec / peak, 4), "traffic": traffic,
                "launches_per_step": dcalls // args.steps, "avg_launch_us": round(1e6 * dsec / dcalls, 2),
                "alg_gflop_per_launch": round(dflops / dcalls / 1e9, 3),
                "share_of_serialized_step": round(dsec / args.steps / t_ser, 3),
                # all convolution FLOPs of a step over the step time of the timed region (every kernel included, not a kernel roofline)
                "whole_step_tflops": round(flops_step / (elapsed / args.steps) / 1e12, 1),
                "measured": "K steps on one stream with an event pair around every launch (kernels alone on the chip), %.2f ms/step; "
                            "the stage times come from a second pass of K steps with stage events only, %.2f ms/step" % (1e3 * t_ser, 1e3 * t_stage),
                "all_conv_classes": {c: {"tflops": round(v[0] / v[1] / 1e12, 2), "calls_per_step": v[2] // args.steps,
                                         "ms_per_step": round(1e3 * v[1] / args.steps, 3)} for c, v in agg.items()}}
    # backbone (stem + res2..res5 + FPN, SURVEY §8d "backbone" column: 287.05 GFLOP per image for R50) over the backbone-only
    # time of the same serialized pass: HIP events around each backbone stage on the launch stream (trace.StageTrace)
    bb = {k: v for k, v in stages.items() if k.startswith("backbone.")}
    if bb:
        bms, bgf = sum(v["ms"] for v in bb.values()) / args.steps, sum(v["gflop"] for v in bb.values()) / args.steps
        roofline["backbone"] = {"achieved": round(bgf / bms, 2), "unit": "TFLOP/s", "frac": round(bgf * 1e9 / (bms * 1e-3) / peak, 4),
                                "ms_per_step": round(bms, 3), "alg_gflop_per_step": round(bgf, 1),
                                "stages": {k[len("backbone."):]: {"ms": round(v["ms"] / args.steps, 3), "tflops": round(v["gflop"] / max(v["ms"], 1e-9), 1)}
                                           for k, v in sorted(bb.items())}}
        # ... and the ResNet trunk alone (stem + res2..res5: 165.25 GFLOP per image for R50), the part furthest from the roofline
        tr = {k: v for k, v in bb.items() if not k.endswith(".fpn")}
        tms, tgf = sum(v["ms"] for v in tr.values()) / args.steps, sum(v["gflop"] for v in tr.values()) / args.steps
        roofline["trunk"] = {"achieved": round(tgf / tms, 2), "unit": "TFLOP/s", "frac": round(tgf * 1e9 / (tms * 1e-3) / peak, 4),
                             "ms_per_step": round(tms, 3), "alg_gflop_per_step": round(tgf, 1)}
        # the same two numbers the way rounds 1 - 4 measured them (stage events in the pass that also brackets every launch)
        bbi = {k: v for k, v in stages_instr.items() if k.startswith("backbone.")}
        for key, sel in (("backbone", bbi), ("trunk", {k: v for k, v in bbi.items() if not k.endswith(".fpn")})):
            ms, gf = sum(v["ms"] for v in sel.values()) / args.steps, sum(v["gflop"] for v in sel.values()) / args.steps
            roofline[key]["with_per_launch_events"] = {"ms_per_step": round(ms, 3), "frac": round(gf * 1e9 / (ms * 1e-3) / peak, 4)}
    roofline["stage_ms_per_step"] = {k: round(v["ms"] / args.steps, 3) for k, v in sorted(stages.items()) if not k.startswith("backbone.")}
    # the 256-cout ring kernel is one source with one template instance (= one rocprofv3 kernel name) per tile height
    fam = [v for c, v in agg.items() if c.startswith("conv_ring_kernel<") and c.endswith("x256>")]
    if fam:
        ff, ft, fc = sum(v[0] for v in fam), sum(v[1] for v in fam), sum(v[2] for v in fam)
        roofline["ring256_family"] = {"tflops": round(ff / ft / 1e12, 2), "frac": round(ff / ft / peak, 4), "calls_per_step": fc // args.steps,
                                      "ms_per_step": round(1e3 * ft / args.steps, 3)}

    # ... and so is the weight-stationary 3x3 kernel (instances per channel count and ReLU flag)
    fam = [v for c, v in agg.items() if c.startswith(("conv3x3_wsr_kernel<", "conv3x3_wsq_kernel<", "conv3x3_ws1_kernel<"))]      # kernel classes 6 and 10
    if fam:
        ff, ft, fc = sum(v[0] for v in fam), sum(v[1] for v in fam), sum(v[2] for v in fam)
        roofline["wsr_family"] = {"tflops": round(ff / ft / 1e12, 2), "frac": round(ff / ft / peak, 4), "calls_per_step": fc // args.steps,
                                  "ms_per_step": round(1e3 * ft / args.steps, 3)}

    # the kernel classes whose roof is HBM (pointwise / fused-bottleneck / stem layers: a few FLOP per byte): ALGORITHMIC bytes (input +
    # output + residual + weights, each once) per second of the same event-timed launches, against 8 TB/s - so that the line shows
    # which part of the backbone sits at its roof (the practical ceiling of a streaming kernel on this chip is 5.5 - 6.3 TB/s) and
    # which part is far from either roof
    hbm = {}
    for c, v in agg.items():
        if v[1] > 0 and c.startswith(("conv1x1_stream_kernel", "bottleneck_tail64_kernel", "bottleneck_pair128_kernel", "stem_pool_kernel",
                                      "conv1x1_pws_kernel", "conv1x1_pwq_kernel")):
            hbm[c] = {"bound": "hbm", "achieved": round(v[3] / v[1] / 1e9, 1), "peak": PEAK_HBM / 1e9, "unit": "GB/s", "frac": round(v[3] / v[1] / PEAK_HBM, 4),
                      "alg_mb_per_step": round(v[3] / args.steps / 1e6, 1), "ms_per_step": round(1e3 * v[1] / args.steps, 3),
                      "calls_per_step": v[2] // args.steps,
                      "tflops": round(v[0] / v[1] / 1e12, 1)}
    roofline["hbm_bound_classes"] = hbm
    # Flat copies of the nested figures a reader of the first level needs (a consumer that keeps only scalars of `roofline` / `config` still sees
    # them), and a cross-check of the event-timed dominant kernel against the newest committed rocprofv3 summary of the same serialized run.
    if traffic:
        roofline["traffic_hbm_bytes_per_launch"] = traffic["hbm_bytes_per_launch"]
        # counter traffic over the kernel's algorithmic bytes per launch (input + weights + output, once each): > 1 = re-reads
        roofline["alg_mb_per_launch"] = round(agg[dom][3] / dcalls / 1e6, 1)
        roofline["traffic_over_algorithmic"] = round(traffic["hbm_bytes_per_launch"] / max(agg[dom][3] / dcalls, 1.0), 3)
    if "backbone" in roofline:
        roofline["backbone_frac"] = roofline["backbone"]["frac"]
        roofline["backbone_ms_per_step"] = roofline["backbone"]["ms_per_step"]
        roofline["backbone_frac_with_per_launch_events"] = roofline["backbone"]["with_per_launch_events"]["frac"]
        roofline["backbone_method"] = ("HIP events around the stem / res2..res5 / FPN stages in a serialized pass WITHOUT per-launch events "
                                       "(rounds 1 - 4 took them from the pass that brackets every launch: backbone_frac_with_per_launch_events)")
        roofline["trunk_frac"] = roofline["trunk"]["frac"]
    for fam_key in ("ring256_family", "wsr_family"):
        if fam_key in roofline:
            roofline[fam_key + "_frac"] = roofline[fam_key]["frac"]
            roofline[fam_key + "_ms_per_step"] = roofline[fam_key]["ms_per_step"]
    rp = rocprof_average_us(dom, args)
    if rp is not None:
        roofline["rocprof_avg_launch_us"] = rp[0]
        roofline["rocprof_source"] = rp[1]
        dev = roofline["avg_launch_us"] / rp[0] - 1.0
        roofline["event_vs_rocprof"] = round(dev, 4)
        if abs(dev) > 0.05:
            roofline["warning"] = ("the event-timed average launch of %s (%.1f us) differs by %+.1f %% from the committed rocprofv3 average (%.1f us, %s): "
                                   "another box / clock than the profile's, or the profile is stale" % (
                                       dom, roofline["avg_launch_us"], 100 * dev, rp[0], rp[1]))

    result = None
    if rank == 0:
        images = args.batch * world * args.steps
        result = {
            "metric": "images/sec at 1/2/4/8 MI355X, R_50_FPN_s1x 800x1333; p50 ms/img" if args.config == "densepose_rcnn_R_50_FPN_s1x"
                      else "images/sec, %s 800x1333" % args.config,
            "value": round(images / elapsed, 3), "unit": "images/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(1e3 * elapsed / args.steps, 3),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": {"bf16": "bf16", "fp16": "f16", "fp32": "f32"}[args.dtype], "data": "synthetic",
            "p50_ms_per_img": round(1e3 * float(np.median(step_times)) / args.batch, 3),
            "p50_note": "p50 of synchronised batch-%d steps divided by %d (throughput-style); p50_single_frame_ms is the batch-1 call latency" % (
                args.batch, args.batch),
            "p50_single_frame_ms": round(1e3 * float(np.median(single_times)), 3) if single_times else None,
            "sustained": sustained, "host_frames": host_rate,
            "config": {"workload": "%s batch=%d/GPU %dx%d uint8 frames resident in HBM, R=%d detections/img (measured %s), synthetic seeded weights"
                                   % (args.config, args.batch, hw[0], hw[1], args.dets, dets),
                       # the reference's own boundary hands over CPU tensors (defaults.py:65-80, run.py:34-36): the same K-step loop with every
                       # frame starting in pageable host memory (pinned ring + copy stream), beside `value` (frames resident in HBM, as the
                       # measurement contract of this benchmark defines it)
                       "images_per_s_host_resident_frames": (host_rate or {}).get("images_per_s"),
                       "images_per_s_sustained": (sustained or {}).get("images_per_s"),
                       "p50_single_frame_ms": round(1e3 * float(np.median(single_times)), 3) if single_times else None,
                       "global_batch": args.batch * world, "parallelism": "frame-sharded dp%d, no hot-loop collective" % world,
                       "alg_gflop_per_image": round(flops_step / args.batch / 1e9, 1),
                       "schedule": "%d batch stream(s), %s, decoder %s, %d pipeline lane(s)"
                                   % (args.streams, "eager launches" if args.no_graphs else "HIP-graph replay of the static part",
                                      "on a side stream" if overlap else "in line", args.pipeline if pipelined else 1)},
            "roofline": roofline,
        }
        if multi is not None:
            if dist_info is not None:
                multi.update(dist_info)
            result["multi_gpu"] = multi
        if world == 1 and not args.no_extras:
            result["accuracy_vs_fp32_reference"] = accuracy_vs_golden(pred, args.dtype) if (
                args.config == "densepose_rcnn_R_50_FPN_s1x" and args.dets == 8 and hw == (800, 1333)) else None
            result["r_sensitivity"] = r_sensitivity(args, state, frames, device)
        if world == 1 and not args.no_cpu_baseline:
            result["cpu_baseline"] = cpu_baseline(cfg, state, hw, args.cpu_budget_s)
        print(json.dumps(result), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
