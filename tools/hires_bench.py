#!/usr/bin/env python3
"""Cost of the hires fix (generate_image(..., hires=...), minsdtf_amd/hires.py) on one GPU, seeded synthetic SD1.5 weights:

  (a) the hand-off kernel (msd_latent_resample, 64x64 -> 128x128 latent, bicubic, with the re-noise): its GPU time from a
      `rocprofv3 --kernel-trace --stats` run of a child process, its per-launch period inside a replayed hipGraph, and the
      ratio of that period to the empty-kernel launch floor tools/launch_floor.py reports on the same box;
  (b) the same hand-off done the host way: device -> host copy, torch's CPU interpolate + re-noise, host -> device copy;
  (c) a 512 -> 1024 hires job (25 + 25 steps at strength 0.6: 15 run): seconds of the first call (both engines recorded, both
      loops captured), images/s of repeated calls, and the two plain jobs it is made of - 25 steps at 512x512 ending in the
      latent (return_latent=True: pass 1 is not decoded either) and `run2` steps at 1024x1024 with the decode, each on a
      pipeline of its own with its engine resident - timed in alternation with it in the same process.
      (With hires=None a job takes the code path it took before the feature, so these two are the figures to compare with.)

    python tools/hires_bench.py --out profiles/hires_bench.json
"""
import argparse
import csv
import glob
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
H1, H2, MODE, A, S = 64, 128, "bicubic", 0.8306, 0.5568


def handoff(dev):
    """(the op's Call, its tensors) for a batch-1 64x64 -> 128x128 hand-off."""
    import torch

    from minsdtf_amd import hires, ops

    x = torch.randn(1, H1, H1, 4, device=dev)
    z = torch.randn(1, H2, H2, 4, device=dev)
    out = torch.empty(1, H2, H2, 4, device=dev)
    rows = torch.from_numpy(hires.pack_rows(*hires.taps(H1, H2, MODE))).to(dev)
    call = ops.latent_resample(x=x, out=out, wx=rows, wy=rows, batch=1, h_in=H1, w_in=H1, h_out=H2, w_out=H2, a=A, s=S, noise=z)
    return call, (x, z, out, rows)


def child_kernel():
    """What the rocprofv3 run executes: 200 launches of the hand-off kernel."""
    import torch

    dev = torch.device("cuda:0")
    call, _keep = handoff(dev)
    st = torch.cuda.current_stream().cuda_stream
    for _ in range(200):
        call(st)
    torch.cuda.synchronize()


def kernel_stats():
    """Average GPU time of latent_resample_kernel (us) from rocprofv3's kernel stats, or None when the profiler is missing."""
    d = tempfile.mkdtemp(prefix="hires_prof_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__),
           "--child-kernel"]
    try:
        subprocess.run(cmd, check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    except (OSError, subprocess.SubprocessError) as e:
        return {"error": f"{type(e).__name__}: {e}"[:300]}
    for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        with open(path) as f:
            for row in csv.DictReader(f):
                if "latent_resample_kernel" in row.get("Name", ""):
                    return {"calls": int(row["Calls"]), "avg_us": round(float(row["AverageNs"]) / 1e3, 3),
                            "min_us": round(float(row["MinNs"]) / 1e3, 3), "max_us": round(float(row["MaxNs"]) / 1e3, 3)}
    return {"error": "latent_resample_kernel not in the kernel stats"}


def graph_period_us(call, n=400):
    import torch

    torch.cuda.synchronize()
    call(torch.cuda.current_stream().cuda_stream)   # (the code object loads outside the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        st = torch.cuda.current_stream().cuda_stream
        for _ in range(n):
            call(st)
    g.replay()
    torch.cuda.synchronize()
    best = 1e30
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) * 1e3 / n)
    del g
    return best


def launch_floor_us():
    """Per-launch period of an empty 256-workgroup kernel in a replayed graph, from tools/launch_floor.py."""
    try:
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "launch_floor.py")], check=True, stdout=subprocess.PIPE,
                             stderr=subprocess.PIPE, text=True, timeout=300).stdout
    except (OSError, subprocess.SubprocessError) as e:
        return None, f"{type(e).__name__}: {e}"[:300]
    m = re.search(r"empty kernel,\s+256 workgroups:\s+([0-9.]+) us", out)
    return (float(m.group(1)), None) if m else (None, "no empty-kernel line")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--child-kernel", action="store_true")
    ap.add_argument("--base", type=int, default=512)
    ap.add_argument("--scale", type=float, default=2.0)
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--strength", type=float, default=0.6)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip-job", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if args.child_kernel:
        return child_kernel()

    import torch
    import torch.nn.functional as F

    from minsdtf_amd import hires, host
    from minsdtf_amd.stable_diffusion import StableDiffusion

    out = {"metric": "hires", "handoff": {"latent": [H1, H2], "upscaler": MODE, "batch": 1}}
    out["a_kernel_rocprofv3"] = kernel_stats()   # (first: a child process, before this one opens the GPU)
    floor, err = launch_floor_us()
    host.fit_torch_threads()
    dev = torch.device("cuda:0")
    call, (x, z, dst, _rows) = handoff(dev)
    period = graph_period_us(call)
    out["a_graph_period_us"] = round(period, 3)
    out["a_launch_floor_us"] = floor if floor is not None else {"error": err}
    if floor:
        out["a_period_over_floor"] = round(period / floor, 3)

    # (b) the host route
    def host_route():
        xh = x.cpu().permute(0, 3, 1, 2)
        up = F.interpolate(xh, size=(H2, H2), mode=MODE, align_corners=False).permute(0, 2, 3, 1)
        dst.copy_((A * up + S * z.cpu()).contiguous())
        torch.cuda.synchronize()

    def device_route():
        call(torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()

    for name, fn in (("b_host_route_us_median", host_route), ("b_device_route_wall_us_median", device_route)):
        fn()
        ts = []
        for _ in range(30):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        out[name] = round(statistics.median(ts) * 1e6, 1)

    if not args.skip_job:
        big = int(round(args.base * args.scale))
        job = hires.parse(dict(scale=args.scale, steps=args.steps, strength=args.strength), args.base, args.base, args.steps)
        rng = np.random.default_rng(0)
        ctx = rng.standard_normal((77, 768)).astype(np.float32)
        unc = rng.standard_normal((77, 768)).astype(np.float32)
        sd = StableDiffusion(args.base, args.base, jit_compile=True, device=dev)
        sd.diffusion_model.load_synthetic(seed=0)
        sd.image_decoder.load_synthetic(seed=0)
        sd.unconditional_context = unc
        kw = dict(batch_size=1, unconditional_guidance_scale=7.5, seed=0, guidance_rescale=0.7)
        hr = dict(scale=args.scale, steps=args.steps, strength=args.strength)

        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        first = timed(lambda: sd.generate_image(ctx, num_steps=args.steps, hires=hr, **kw))
        # the two plain jobs, each on its own pipeline (so its engine stays resident), over the same packed weights
        lo = StableDiffusion(args.base, args.base, jit_compile=True, device=dev)
        hi = StableDiffusion(big, big, jit_compile=True, device=dev)
        lo._diffusion_model = sd.diffusion_model
        hi._diffusion_model = sd._unet_for(big, big)
        for p in (lo, hi):
            p._image_decoder, p.unconditional_context = sd.image_decoder, unc
        jobs = {
            "hires": lambda: sd.generate_image(ctx, num_steps=args.steps, hires=hr, **kw),
            "plain_base": lambda: lo.generate_image(ctx, num_steps=args.steps, return_latent=True, **kw),   # (pass 1 ends undecoded)
            "plain_target": lambda: hi.generate_image(ctx, num_steps=job.run_steps, **kw),
        }
        for fn in jobs.values():
            fn()   # warm: engines built, loops captured, decoder plans bound
        times = {k: [] for k in jobs}
        for _ in range(args.rounds):
            for k, fn in jobs.items():
                times[k].append(timed(fn))
        med = {k: statistics.median(v) for k, v in times.items()}
        parts = med["plain_base"] + med["plain_target"]
        out["c_job"] = {"base": args.base, "target": big, "steps": [args.steps, job.steps], "strength": args.strength,
                        "run_steps": [args.steps, job.run_steps], "rounds": args.rounds}
        out["c_first_call_s"] = round(first, 3)
        out["c_repeat_s_median"] = round(med["hires"], 4)
        out["c_repeat_images_per_s"] = round(1.0 / med["hires"], 4)
        out["c_first_over_repeat"] = round(first / med["hires"], 2)
        out["c_plain_base_s_median"] = round(med["plain_base"], 4)       # (return_latent=True: no decode, as pass 1)
        out["c_plain_target_s_median"] = round(med["plain_target"], 4)
        out["c_hires_over_sum_of_parts"] = round(med["hires"] / parts, 4)
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
