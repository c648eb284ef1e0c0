#!/usr/bin/env python
"""bench.py -- optimisation iterations/sec of the pixray hot path on MI355X.

One "step" = one body of the reference's train() (pixray.py:1448-1487, batches=1): drawer.synth -> MakeCutouts
(host-drawn augmentation parameters, device noise) -> CLIP encode_image -> Prompt loss (+ custom losses) -> backward ->
(N>1: all-reduce of dL/d(image)) -> Adam -> clip_z, with seeded random weights of the real architectures.

    python bench.py                                  # BASELINE.json configs[1] (the metric): vqgan 256^2 + ViT-B/32 + 64 cutouts
    python bench.py --config cfg2                    # configs[2]: vqgan 512^2 + ViT-B/16 + RN50x4, 128 cutouts per perceptor
    python bench.py --config cfg2 --cutn 16          #   ... at the 16-cutout shard one of 8 GPUs holds
    python bench.py --config cfg3                    # configs[3]: fft 512^2 + ViT-L/14 + 256 cutouts + StyleLoss + SaturationLoss
    python bench.py --precision bf16|f32             # bf16 operands / the exact-f32 MFMA parity mode instead of the fp16 default
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

Prints ONE JSON line on rank 0.  `roofline` is measured live with HIP events around every launch of the dominant kernel
family (the MFMA GEMM / implicit-GEMM conv engine) on the launch stream; `cpu_baseline` times the CPU oracle (a port: the
reference itself is not importable offline) on the host cores, on a stated, bounded sample.
"""
import argparse
import json
import os
import sys
import time

# before anything touches the GPU: hipGraph replay is only safe with the runtime's graph packet capture off (pixray_amd/__init__.py)
os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")
ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# dense MFMA peaks, /opt/skills/guides/MI355X_MICROARCH.md
PEAK_TFLOPS = {"fp16": 2500.0, "bf16": 2500.0, "f32": 157.3, "ref": 2500.0}
# algorithmic work per iteration at the headline config; the other configurations report
# the contraction flops the engine executed (sum of 2MNK over its launches, split-K counted once)
GFLOP_DECODER_256 = 506.0 + 2.1
GFLOP_CLIP_B32_PER_CUT = 8.82 + 8.91


def make_saturation_loss(device):
    """BASELINE.json configs[3]'s SaturationLoss: the reference plugin is plain torch (Losses/SaturationLoss.py:15-30) and
    drops in unchanged where /root/reference exists (tests/test_host_logic.py); the GPU box has no reference tree, so the
    benchmark carries the same arithmetic as a LossInterface plugin of its own."""
    import torch
    from pixray_amd.interfaces import LossInterface

    class SaturationLoss(LossInterface):
        needs_full_batch = True          # std over ALL cutout pixels: scored on the gathered batch when sharded
        supports_graph_replay = True     # device tensors in, device tensors out: no host draw, upload or branch

        def get_loss(self, cur_cutouts, out, args, globals=None, lossGlobals=None):
            res = []
            for _, cutouts in cur_cutouts.items():
                px = cutouts.permute(0, 2, 3, 1).reshape(-1, 3)
                rg, yb = px[:, 0] - px[:, 1], 0.5 * (px[:, 0] + px[:, 1]) - px[:, 2]
                rg_std, rg_mean = torch.std_mean(rg)
                yb_std, yb_mean = torch.std_mean(yb)
                res.append(-(torch.sqrt(rg_std ** 2 + yb_std ** 2) + 0.3 * torch.sqrt(rg_mean ** 2 + yb_mean ** 2)) / 10.0)
            return res
    return SaturationLoss(device=device)


def cfg3_custom_losses(device, precision, on_cpu=False):
    """StyleLoss (VGG16 extractor on the HIP engine, STROTSS on top) + SaturationLoss, synthetic style image and VGG weights.
    --styleloss_skip 0: the steady state after the reference's default 100 silent iterations."""
    import argparse as ap
    import torch
    from pixray_amd import style_loss as sl
    from pixray_amd import weights
    args = sl.StyleLoss.add_settings(ap.ArgumentParser()).parse_args(["--styleloss_skip", "0"])
    params = weights.synthetic_vgg16_params(0)
    style_img = torch.rand(1, 3, 384, 448, generator=torch.Generator().manual_seed(4))
    if on_cpu:
        from oracle import workload_ref
        style = sl.StyleLoss(extractor=workload_ref.OracleVggExtractor(params), style_image=style_img, device="cpu",
                             reference_schedule=True)
        sat = workload_ref.SaturationLossRef()
    else:
        from pixray_amd._lib import split_precision
        ext = sl.Vgg16Extractor(space=args.styleloss_ospace, params=params, device=device, max_hw=(512, 512),
                                precision=split_precision(precision)[1])
        style = sl.StyleLoss(extractor=ext, style_image=style_img, device=device)
        sat = make_saturation_loss(device)
    args = style.parse_settings(args)
    return [{"loss": style, "weight": 1.0}, {"loss": sat, "weight": 1.0}], args


class CollectiveTimer:
    """per-collective device time of the N>1 path: wraps torch.distributed's all_reduce / all_gather with events"""

    def __init__(self):
        self.records = []
        self._orig = {}

    def __enter__(self):
        import torch
        import torch.distributed as dist
        for name in ("all_reduce", "all_gather"):
            orig = getattr(dist, name)
            self._orig[name] = orig

            def wrapped(*a, _orig=orig, _name=name, **k):
                t = a[0] if _name == "all_reduce" else a[1]
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                r = _orig(*a, **k)
                e1.record()
                self.records.append((f"{_name}[{t.numel() * t.element_size()} B]", e0, e1))
                return r
            setattr(dist, name, wrapped)
        return self

    def __exit__(self, *exc):
        import torch.distributed as dist
        for name, orig in self._orig.items():
            setattr(dist, name, orig)

    def summary(self, steps):
        out = {}
        for key, e0, e1 in self.records:
            out[key] = out.get(key, 0.0) + e0.elapsed_time(e1)
        return {k: round(v / steps, 4) for k, v in out.items()}


DUMP_MAX_BYTES = 64 << 20


def dump_outputs(sess, it, out_dir):
    """What the last timed step hands its caller, as <out_dir>/<name>.npy: the loss terms (`loss_terms`, float64), every
    parameter the optimisers update, after the step and clip_z (`param<i>`), its gradient from that step's backward
    (`param<i>_grad`), and the image the updated parameters render (`image`, drawer.synth without autograd).  Arrays are float32
    except the losses; one larger than its share of the 64 MB budget is replaced by a fixed, seeded sample of its flattened
    values.  The same arguments give the same inputs, so two builds can be compared file for file."""
    import numpy as np
    import torch
    arrays = {"loss_terms": np.concatenate([np.asarray(l.detach().double().cpu() if isinstance(l, torch.Tensor) else l,
                                                       dtype=np.float64).ravel() for l in sess.last_losses])}
    params = [p for opt in sess.opts for g in opt.param_groups for p in g["params"]]
    for i, p in enumerate(params):
        arrays[f"param{i}"] = p.detach().float().cpu().numpy()
        if p.grad is not None:
            arrays[f"param{i}_grad"] = p.grad.detach().float().cpu().numpy()
    with torch.no_grad():
        arrays["image"] = sess.drawer.synth(it).detach().float().cpu().numpy()
    os.makedirs(out_dir, exist_ok=True)
    share = DUMP_MAX_BYTES // len(arrays)
    for name, a in arrays.items():
        if a.nbytes > share:
            idx = np.sort(np.random.default_rng(0).choice(a.size, share // a.itemsize, replace=False))
            a = a.reshape(-1)[idx]
        np.save(os.path.join(out_dir, f"{name}.npy"), a)
    return list(arrays)


def spawn_command(n, argv, port=None):
    """the command line `python bench.py --gpus n` re-executes itself under (one rank per GPU of this node over RCCL)"""
    import socket
    if port is None:
        with socket.socket() as so:              # a free rendezvous port on the loopback interface
            so.bind(("127.0.0.1", 0))
            port = so.getsockname()[1]
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
            "--master-port", str(port), os.path.abspath(__file__)] + list(argv)


def spawn_ranks(n, argv):
    import subprocess
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")     # RCCL / IPC handles need the dmabuf path on this driver
    return subprocess.call(spawn_command(n, argv), env=env)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=None)
    ap.add_argument("--config", choices=["cfg1", "cfg2", "cfg3"], default="cfg1")
    ap.add_argument("--cutn", type=int, default=None, help="cutouts (default: the configuration's own count)")
    ap.add_argument("--precision", choices=["fp16", "bf16", "f32", "ref"], default="fp16",
                    help="operand precision of the timed run: ref = the reference's own mix on a GPU (fp32 VQGAN decoder on the exact-f32 "
                         "MFMA + fp16 CLIP towers; cfg1 / cfg2), fp16 (default; the reference's own GPU arithmetic for CLIP, slip.py:175), "
                         "bf16, or f32 (exact-f32 MFMA parity mode)")
    ap.add_argument("--no-other-modes", action="store_true",
                    help="skip the extra legs (headline config, 1 GPU): it/s of the other precisions and dL/dz parity of every mode")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--graph", dest="graph", action="store_true", default=None,
                    help="replay the iteration from a captured hipGraph.  Default: on for cfg3 (its StyleLoss plugin is bound by the "
                         "host's launch rate when launched eagerly), off for cfg1 / cfg2 (measured neutral: GPU-bound)")
    ap.add_argument("--no-graph", dest="graph", action="store_false")
    ap.add_argument("--cpu-iters", type=int, default=3)
    ap.add_argument("--cpu-sample-cutn", type=int, default=None)
    ap.add_argument("--profile-steps", type=int, default=3)
    ap.add_argument("--phase-steps", type=int, default=2, help="iterations of the synchronised phase breakdown (0: skip)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step computed as DIR/<name>.npy (rank 0): the loss "
                         "terms, the drawer's parameters after the optimiser step, their gradients and the image they render")
    ap.add_argument("--dry-run", action="store_true",
                    help="launch mechanics only: every rank joins a gloo group on the host, rank 0 prints {world, ranks} and exits "
                         "(CPU test of the bare `--gpus N` form; no GPU touched)")
    args = ap.parse_args()
    if args.steps is not None and args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.warmup is not None and args.warmup < 0:
        ap.error("--warmup must not be negative")

    if args.dry_run:
        if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
            raise SystemExit(spawn_ranks(args.gpus, sys.argv[1:]))
        import torch.distributed as dist
        world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
        seen = [rank]
        if world > 1:
            dist.init_process_group("gloo", rank=rank, world_size=world)
            seen = [None] * world
            dist.all_gather_object(seen, rank)
            dist.destroy_process_group()
        if rank == 0:
            print(json.dumps({"dry_run": True, "world": world, "ranks": sorted(seen), "gpus": args.gpus}), flush=True)
        return

    import torch
    from pixray_amd import _lib, api

    wl = api.WORKLOADS[args.config]
    cutn = args.cutn if args.cutn else wl["num_cuts"]
    heavy = args.config != "cfg1" or args.precision in ("f32", "ref")
    steps = args.steps if args.steps is not None else (10 if heavy else 30)
    warmup = args.warmup if args.warmup is not None else (2 if heavy else 5)

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # launched bare (`python bench.py --gpus N`): start the N ranks ourselves, one process per GPU, exactly as the driver's
        # `python -m torch.distributed.run --nnodes=1 --nproc-per-node N ...` form does; rank 0 prints the JSON line
        raise SystemExit(spawn_ranks(args.gpus, sys.argv[1:]))
    if args.gpus > 1 and world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} needs WORLD_SIZE={args.gpus} (got {world}): launch with "
                         f"`python -m torch.distributed.run --nnodes=1 --nproc-per-node {args.gpus} bench.py --gpus {args.gpus} ...` "
                         f"or bare `python bench.py --gpus {args.gpus}`")
    # PRX_ONE_DEVICE=1 + PRX_DIST_BACKEND=gloo: every rank on cuda:0 with the host-side bootstrap on gloo and ALL THREE collectives
    # of the iteration on the C-ABI one-shot exchange (csrc/comm.hip) -- how the multi-rank path is exercised end to end where
    # only one GPU is reachable (RCCL refuses two ranks on one device; the exchange does not care where the peer window lives)
    one_device = os.environ.get("PRX_ONE_DEVICE") == "1"
    backend = os.environ.get("PRX_DIST_BACKEND", "nccl")
    if one_device:
        local_rank = 0
    if backend != "nccl":
        os.environ["PRX_ONESHOT_ALLREDUCE"] = "1"          # gloo carries the bootstrap and the barriers only
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    group = None
    force_dist = os.environ.get("PRX_FORCE_DIST") == "1"      # exercise the RCCL code path on a single GPU
    if world > 1 or force_dist:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
        group = dist.group.WORLD
    torch.manual_seed(1234 + rank)          # per-rank device noise streams (host-side draws are seeded identically)

    custom, largs = ((), None)
    if args.config == "cfg3":
        import numpy as np
        np.random.seed(0)                    # STROTSS samples its hyper-column positions from numpy's global RNG
        custom, largs = cfg3_custom_losses(dev, args.precision)
    sess = api.build_workload(args.config, num_cuts=cutn, precision=args.precision, device=dev, group=group, rank=rank,
                              world_size=world, custom_losses=custom, args=largs)
    if force_dist and world == 1:
        sess.world_size = 1
        for p_ in sess.perceptors.values():
            p_.group = group              # min/max + renorm-gradient all-reduces over the 1-rank group
        sess._force_hook_group = group

    def barrier():
        if world > 1 or force_dist:
            import torch.distributed as dist
            dist.barrier(group=group)
        torch.cuda.synchronize(dev)

    it = 0
    graphed = False
    if args.graph is None:
        args.graph = args.config == "cfg3"
    if args.graph and (world == 1 or getattr(sess, "comm", None) is not None):   # N > 1: only on the capturable one-shot exchange (engine.enable_graph)
        graphed = sess.enable_graph(warmup=max(warmup - 1, 1))      # warm-up iterations run inside
        it = sess.cur_iteration
    for _ in range(0 if graphed else warmup):
        sess.train(it); it += 1
    barrier()
    t0 = time.perf_counter()
    for _ in range(steps):
        sess.train(it); it += 1
    barrier()
    elapsed = time.perf_counter() - t0
    if world > 1:
        import torch.distributed as dist
        t = torch.tensor([elapsed], device=dev if backend == "nccl" else "cpu", dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX, group=group)
        elapsed = float(t.item())
    ms_per_step = 1e3 * elapsed / steps
    value = steps / elapsed
    loss = float(sum(l.detach() for l in sess.last_losses))
    if world > 1:      # a rank's terms are its shard's share (weight / world) of the prompt losses: the step's loss is their sum over ranks
        import torch.distributed as dist
        lt = torch.tensor([loss], device=dev if backend == "nccl" else "cpu", dtype=torch.float64)
        dist.all_reduce(lt, op=dist.ReduceOp.SUM, group=group)
        loss = float(lt.item())
    if args.dump_outputs and rank == 0:
        names = dump_outputs(sess, it, args.dump_outputs)
        print(f"bench.py: wrote {', '.join(names)} to {args.dump_outputs}", file=sys.stderr, flush=True)

    # ---- per-collective device time (N > 1, or the forced 1-rank group) ------------------------------------------------
    collectives = None
    if world > 1 or force_dist:
        with CollectiveTimer() as ct:
            for _ in range(args.profile_steps):
                sess.train(it); it += 1
            torch.cuda.synchronize(dev)
        collectives = ct.summary(args.profile_steps)

    # ---- roofline leg: per-launch HIP-event timing of the GEMM engine over a few extra steps ------------------
    # (eager launches: events cannot be recorded around the nodes of a replayed graph)
    roofline = None
    sess._drop_graph()
    peak = PEAK_TFLOPS[args.precision]
    gemm_gflop_step = None
    if rank == 0:
        prof = api.GemmProfile(sess)
        prof.enable(True)
        for _ in range(args.profile_steps):
            sess.train(it); it += 1
        torch.cuda.synchronize(dev)
        prof.enable(False)
        raw_ms, flop, n = prof.collect()
        # A bracket [event, kernel, event] also times the events' own timestamp packets.  An EMPTY bracket on this stream
        # measures ~5 us; around a kernel about half of that is hidden behind the kernel's own dispatch/drain, and taking
        # half of the empty-bracket time off every launch reproduces rocprofv3's kernel durations for the same command
        # within 2 % (profiles/r01_e_3stage_c64_kernel_stats.csv: 22.4 us per launch incl. split-K reduce passes).
        pairs = []
        for _ in range(200):
            a_, b_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a_.record(); b_.record(); pairs.append((a_, b_))
        torch.cuda.synchronize(dev)
        ev_over_ms = 0.5 * sorted(x.elapsed_time(y) for x, y in pairs)[len(pairs) // 2]
        if raw_ms > 0 and n > 0:
            ms = max(raw_ms - ev_over_ms * n, 0.5 * raw_ms)
            gemm_gflop_step = flop / args.profile_steps / 1e9
            # ALGORITHMIC work of the engine = what the reference's op list contracts.  The ViT runner's class-token tail does not
            # launch 6 of the last block's 8 wide products on the n * (T - 1) rows nobody reads (csrc/vit.hip); they stay counted
            tail_gflop = 0.0
            for p_ in sess.perceptors.values():
                c_ = getattr(p_, "cfg", None)
                if c_ is not None and hasattr(c_, "patch_size") and getattr(c_, "layers", 0) > 0:
                    n_loc = cutn // world
                    T_ = (c_.input_resolution // c_.patch_size) ** 2 + 1
                    tail_gflop += 2 * 2.0 * (n_loc * T_ - n_loc) * (c_.width ** 2 + 2 * 4 * c_.width ** 2) / 1e9
            gemm_gflop_alg = gemm_gflop_step + tail_gflop
            # `achieved` / `frac` = what the matrix pipes DID: launched flops over the launches' time.  The algorithmic figure (with the
            # products the class-token tail skips) is reported beside it as an MFU-style field, not as the roofline fraction
            achieved = gemm_gflop_step * args.profile_steps * 1e9 / (ms * 1e-3) / 1e12
            achieved_alg = gemm_gflop_alg * args.profile_steps * 1e9 / (ms * 1e-3) / 1e12
            kern = (f"GEMM engine: gemmfit_kernel<WGM,WGN,FM,FN,KS,CONV> + gemm_glds_kernel / gemm8p_kernel / gemmrow_kernel / gemmrowconv_kernel ({args.precision} MFMA GEMM / implicit 3x3 conv, all launches)"
                    if args.precision != "f32"
                    else "gemm_f32_kernel<BM,BN,AMODE> (v_mfma_f32_32x32x2_f32 GEMM / implicit 3x3 conv, all launches)")
            # HBM-side bytes per launch come from rocprofv3 PMC passes (separate --pmc FETCH_SIZE / WRITE_SIZE runs of this
            # command, gfx950 FETCH correction applied): not measurable from inside this process, so `traffic` is null here
            # and the committed profile of the round is quoted next to it when there is one for this configuration
            pmc = None
            pmc_path = next((q for q in (os.path.join(ROOT, "profiles", f"r{rr:02d}_{args.config}_hbm_traffic.json") for rr in (6, 5, 4, 3, 2))
                             if os.path.exists(q)), "")
            if args.precision != "f32" and pmc_path:
                with open(pmc_path) as f:
                    pmc = json.load(f)
                pmc["source"] = os.path.relpath(pmc_path, ROOT)
                pmc["measured_in_this_run"] = False      # a committed rocprofv3 --pmc profile of the same command, not this process
            # `traffic`: HBM-side bytes per launch of this kernel family from the committed PMC passes of this command (FETCH_SIZE
            # and WRITE_SIZE in separate rocprofv3 --pmc runs, gfx950 corrections applied: tools/profile_run.sh, tools/pmc_summary.py);
            # the counters cannot be read from inside the process, so the number is the profile's, with its source beside it
            traffic = round(float(pmc["bytes_per_launch"])) if pmc and pmc.get("bytes_per_launch") else None
            roofline = {"bound": "mfma", "kernel": kern, "achieved": round(achieved, 1), "peak": peak, "unit": "TFLOP/s",
                        "frac": round(achieved / peak, 4), "traffic": traffic,
                        "traffic_unit": "bytes per launch (HBM-side fetch + write), from the committed PMC profile named in traffic_pmc_profile.source -- NOT measured in this run" if traffic else None,
                        "traffic_pmc_profile": pmc,
                        "achieved_algorithmic": round(achieved_alg, 1), "frac_algorithmic": round(achieved_alg / peak, 4),
                        "launches_per_step": n // args.profile_steps,
                        "gemm_gflop_per_step": round(gemm_gflop_alg, 1),
                        "gemm_gflop_launched_per_step": round(gemm_gflop_step, 1),
                        "gemm_ms_per_step": round(ms / args.profile_steps, 3),
                        "avg_launch_us": round(1e3 * ms / max(n, 1), 2),
                        "event_overhead_us_removed_per_launch": round(1e3 * ev_over_ms, 2),
                        "avg_launch_us_raw_events": round(1e3 * raw_ms / max(n, 1), 2)}
    elif world > 1:
        for _ in range(args.profile_steps):      # keep ranks in lock-step through the collectives
            sess.train(it); it += 1

    # ---- phase breakdown (forward phases bracketed by synchronisations; after the timed region, rank 0 only) ----
    phase_ms = None
    if rank == 0 and world == 1 and args.phase_steps > 0:
        phase_ms = api.phase_breakdown(sess, it, args.phase_steps)
        it += args.phase_steps

    if args.config == "cfg1":
        per_gpu_gflop = GFLOP_DECODER_256 + GFLOP_CLIP_B32_PER_CUT * cutn / world
    else:
        per_gpu_gflop = gemm_gflop_step      # rank 0's executed contraction flops (identical on every rank)
    iter_frac = value * per_gpu_gflop * 1e9 / (peak * 1e12) if per_gpu_gflop else None

    # ---- the other operand precisions at the same configuration, and dL/dz parity of every mode against the CPU oracle ----
    # (headline configuration, one GPU, after the timed region; the oracle iteration is ONE extra evaluation on the host)
    other_modes = parity = None
    if rank == 0 and world == 1 and args.config == "cfg1" and cutn == wl["num_cuts"] and not args.no_other_modes and not force_dist:
        del prof
        sess = None
        torch.cuda.empty_cache()
        other_modes = {}
        for prec in ("fp16", "ref", "bf16", "f32"):
            if prec == args.precision:
                continue
            s2 = api.build_workload(args.config, num_cuts=cutn, precision=prec, device=dev)
            n2, w2 = (10, 2) if prec == "f32" else (steps, warmup)      # the like-for-like "ref" leg runs the timed leg's step count
            for i in range(w2):
                s2.train(i)
            torch.cuda.synchronize(dev)
            t1 = time.perf_counter()
            for i in range(n2):
                s2.train(w2 + i)
            torch.cuda.synchronize(dev)
            dt = time.perf_counter() - t1
            other_modes[prec] = {"value": round(n2 / dt, 3), "unit": "iterations/s", "ms_per_step": round(1e3 * dt / n2, 3), "steps": n2,
                                 "warmup": w2,
                                 # "ref" mixes two MFMA peaks: against the ceiling 1 / (decoder GFLOP / f32 peak + tower GFLOP / fp16 peak)
                                 "frac_of_mfma_peak": round((n2 / dt) * ((GFLOP_DECODER_256 * 1e9) / (PEAK_TFLOPS["f32"] * 1e12) + (GFLOP_CLIP_B32_PER_CUT * cutn * 1e9) / (PEAK_TFLOPS["fp16"] * 1e12)), 4)
                                 if prec == "ref" else round((n2 / dt) * per_gpu_gflop * 1e9 / (PEAK_TFLOPS[prec] * 1e12), 4)}
            del s2
            torch.cuda.empty_cache()
        if not args.no_cpu_baseline:
            from oracle import workload_ref
            prm = workload_ref.draws_for(args.config, cutn, 0)
            ref = None
            parity = {"what": "dL/dz after ONE iteration vs the fp32 CPU oracle, same seeds and explicit augmentation draws "
                              "(SURVEY.md 8d gates: f32 rel-L2 <= 1e-4 jitter off / 1e-3 on; fp16, bf16 rel-L2 <= 2e-2 and cosine >= 0.999)"}
            for prec in ("fp16", "ref", "bf16", "f32"):
                hip = workload_ref.hip_gradient(args.config, cutn, prec, prm, 0, str(dev))
                if ref is None:
                    ref = workload_ref.iteration(args.config, cutn, 0, prm, state=hip["start"])
                c = workload_ref.compare_with(ref, hip)
                parity[prec] = {"dz_rel_l2": float(f"{c['grad_rel_l2']:.3e}"), "dz_cosine": round(c["grad_cosine"], 7),
                                "loss_abs_err": float(f"{c['loss_abs_err']:.2e}")}

    cpu_baseline = None
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        from oracle import step_ref, workload_ref
        if args.config == "cfg1":
            r = step_ref.time_oracle_iterations(n_iters=args.cpu_iters, warmup=1, cutn=cutn)
            cpu_baseline = {"value": round(r["iters_per_sec"], 4), "unit": "iterations/s", "cores": r["threads"],
                            "kind": "port",
                            "sample": f"{args.cpu_iters} full iterations (same config, fp32 torch CPU oracle, "
                                      f"{r['threads']} threads of {r['cores']} host cores) after 1 warm-up"}
        else:
            sample = args.cpu_sample_cutn or (16 if args.config == "cfg2" else 8)
            sample = min(sample, cutn)
            ccustom, cargs = ((), None)
            if args.config == "cfg3":
                ccustom, cargs = cfg3_custom_losses("cpu", "f32", on_cpu=True)
            r = workload_ref.time_workload(args.config, sample, n_iters=args.cpu_iters, warmup=1, custom=ccustom, args=cargs)
            # the cutout-proportional part (cutouts + towers) scales linearly in the cutout count; the drawer and the losses
            # that read only the image (StyleLoss) do not
            t_full = r["fixed_seconds"] + (r["seconds_per_iter"] - r["fixed_seconds"]) * (cutn / sample)
            cpu_baseline = {"value": round(1.0 / t_full, 5), "unit": "iterations/s", "cores": r["threads"], "kind": "port",
                            "sample": f"{args.cpu_iters} oracle iterations at {sample} of {cutn} cutouts per perceptor "
                                      f"({r['seconds_per_iter']:.1f} s each, of which drawer + image-only losses {r['fixed_seconds']:.1f} s; fp32 torch, "
                                      f"{r['threads']} threads of {r['cores']} host cores) after 1 warm-up, the cutout-proportional "
                                      f"part extrapolated linearly to {cutn}"}

    if rank == 0:
        metric = {"cfg1": "optimisation iters/sec, VQGAN 256^2 + ViT-B/32 + 64 cutouts",
                  "cfg2": "optimisation iters/sec, VQGAN 512^2 + ViT-B/16 + RN50x4 + 128 cutouts",
                  "cfg3": "optimisation iters/sec, fft 512^2 + ViT-L/14 + 256 cutouts + StyleLoss + SaturationLoss"}[args.config]
        out = {
            "metric": metric,
            "value": round(value, 3), "unit": "iterations/s", "n_gpus": world, "steps": steps,
            "warmup": warmup, "ms_per_step": round(ms_per_step, 3), "higher_is_better": True,
            "scaling": "strong", "vs_baseline": None, "dtype": args.precision, "data": "synthetic",
            "config": {"workload": wl["text"] if cutn == wl["num_cuts"] else wl["text"] + f" [run at {cutn} cutouts per perceptor]",
                       "weights": "seeded random, real architectures", "cutouts_per_gpu": cutn // world,
                       "parallelism": f"cutout-sharded x{world}, all-reduce of dL/d(image)" if world > 1 else "single GPU",
                       "exchange": (None if world == 1 else
                                    ("C-ABI one-shot direct-write all-reduce (prx_allreduce, csrc/comm.hip) for all three collectives"
                                     if getattr(sess, "comm", None) is not None or os.environ.get("PRX_ONESHOT_ALLREDUCE") == "1"
                                     else "RCCL through torch.distributed (nccl)") + (", every rank on ONE device (protocol test)" if one_device else "")),
                       "launch": "hipGraph replay" if graphed else ("eager" + (f" (replay refused: {sess.graph_error})" if args.graph and getattr(sess, "graph_error", None) else "")),
                       "precision": {"fp16": "IEEE-half MFMA operands (v_mfma_f32_32x32x16_f16: the reference's CLIP arithmetic on a GPU), "
                                             "fp32 accumulate and norm arithmetic, residual / feature-map streams and their gradients held in half (the lean layout: slip.py:175 runs the CLIP model in fp16, residual adds included; the fp32 VQGAN of the reference is the `ref` mode), power-of-two gradient scale in the backward",
                                     "bf16": "bf16 MFMA operands, fp32 accumulate / residual streams / norms",
                                     "f32": "exact f32: every contraction on v_mfma_f32_32x32x2_f32 (parity mode)",
                                     "ref": "the reference's own mix on a GPU: fp32 VQGAN decoder (every decoder contraction on "
                                            "v_mfma_f32_32x32x2_f32, vqgan.py:124-140) + IEEE-half CLIP tower (slip.py:175)"}[args.precision]},
            "final_loss": round(loss, 5),
            "per_gpu_gflop_per_step": round(per_gpu_gflop, 1) if per_gpu_gflop else None,
            "iter_mfma_frac": round(iter_frac, 4) if iter_frac else None,
            "roofline": roofline, "cpu_baseline": cpu_baseline, "other_precisions": other_modes, "parity_vs_oracle": parity,
            "collectives_ms_per_step": collectives, "phase_ms": phase_ms,
        }
    if world > 1 or force_dist:
        import torch.distributed as dist
        dist.destroy_process_group()      # RCCL prints its version banner here: keep the JSON line last
    sys.stderr.flush()
    try:                                   # RCCL writes its banner through C stdio: drain it before the JSON line
        import ctypes
        ctypes.CDLL(None).fflush(None)
    except Exception:
        pass
    if rank == 0:
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
