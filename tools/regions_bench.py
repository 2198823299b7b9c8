#!/usr/bin/env python3
"""Cost of regional prompting (generate_image(..., regions=...), minsdtf_amd/regions.py) on one GPU, seeded synthetic SD1.5 weights:

  (a) the combine launch (msd_region_combine; default: 2 regions x 2 samples of a 64 x 64 latent, in place, as the engine records
      it): its per-launch period inside a replayed hipGraph, next to the empty-kernel launch floor tools/launch_floor.py reports
      on the same box;
  (b) the same combine composed from torch ops (one multiply, then one addcmul per further region): its period inside a replayed
      graph and its number of kernel launches - both forms measured in this one process;
  (c) the regional job (R regions, batch B: (1 + R) * B UNet rows per step) against the plain job of the same number of UNet
      rows (batch (1 + R) * B / 2; both end in the latent: the loops are what is compared), the plain job twice (A/A), the three
      timed in alternation in this one process.  The regional job should cost the plain job plus its combine launches, minus
      nothing: regional / plain is to be read against the A/A spread and (a) x steps.

    python tools/regions_bench.py --out profiles/regions_bench.json
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def graph_period_us(fn, n=200):
    """Per-call period of `fn(stream)` repeated n times inside one replayed graph (best of 5 replays)."""
    import torch

    fn(torch.cuda.current_stream())   # (code objects load outside the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            for _ in range(n):
                fn(torch.cuda.current_stream())
    torch.cuda.current_stream().wait_stream(s)
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
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--regions", type=int, default=2)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip-job", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    R, B = args.regions, args.batch
    if ((1 + R) * B) % 2:
        ap.error("(1 + regions) * batch must be even: the plain job of the same UNet rows has batch (1 + regions) * batch / 2")

    floor, err = launch_floor_us()   # (first: a child process, before this one opens the GPU)
    import torch

    from minsdtf_amd import host, ops, regions
    from minsdtf_amd.stable_diffusion import StableDiffusion

    host.fit_torch_threads()
    dev = torch.device("cuda:0")
    h = w = args.size // 8
    n = h * w * 4
    masks = regions.boxes(h, w, 1, R)
    out = {"metric": "regions", "shape": {"size": args.size, "regions": R, "batch": B, "unet_rows": (1 + R) * B}}

    # (a) the launch, (b) the torch composition of it
    eps = torch.randn(R * B, n, device=dev)
    wt = torch.from_numpy(regions.weights(masks)).to(dev)
    call = ops.region_combine(eps=eps, w=wt, out=eps, regions=R, batch=B, n=n)
    e5 = eps.view(R, B, h, w, 4)
    w5 = wt.view(R, 1, h, w, 1)
    launches = [0]

    def torch_route(_stream):
        torch.mul(e5[0], w5[0], out=e5[0])
        for r in range(1, R):
            e5[0].addcmul_(e5[r], w5[r])
        launches[0] = R

    period = graph_period_us(lambda st: call(st.cuda_stream))
    torch_period = graph_period_us(torch_route, n=50)
    out["a_graph_period_us"] = round(period, 3)
    out["a_launch_floor_us"] = floor if floor is not None else {"error": err}
    if floor:
        out["a_period_over_floor"] = round(period / floor, 3)
    out["b_torch_ops_graph_period_us"] = round(torch_period, 3)
    out["b_torch_ops_launches"] = launches[0]
    out["b_torch_over_kernel"] = round(torch_period / period, 2)

    if not args.skip_job:
        rng = np.random.default_rng(0)
        ctx = rng.standard_normal((77, 768)).astype(np.float32)
        unc = rng.standard_normal((77, 768)).astype(np.float32)
        job = dict(regions=[dict(prompt=rng.standard_normal((77, 768)).astype(np.float32), mask=m) for m in masks])
        pipes = []
        for _ in range(3):   # one pipeline per timed job, so each keeps its engine resident; one set of packed weights
            p = StableDiffusion(args.size, args.size, jit_compile=True, device=dev)
            if pipes:
                p._diffusion_model = pipes[0].diffusion_model
            else:
                p.diffusion_model.load_synthetic(seed=0)
            p.unconditional_context = unc
            pipes.append(p)
        kw = dict(num_steps=args.steps, unconditional_guidance_scale=7.5, seed=0, guidance_rescale=0.7, return_latent=True)
        PB = (1 + R) * B // 2

        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        jobs = {
            "regional": lambda: pipes[0].generate_image(ctx, batch_size=B, regions=job, **kw),
            "plain": lambda: pipes[1].generate_image(ctx, batch_size=PB, **kw),
            "plain_again": lambda: pipes[2].generate_image(ctx, batch_size=PB, **kw),
        }
        first = timed(jobs["regional"])
        for fn in jobs.values():
            fn()   # warm: engines built, loops captured
        times = {k: [] for k in jobs}
        for _ in range(args.rounds):
            for k, fn in jobs.items():
                times[k].append(timed(fn))
        med = {k: statistics.median(v) for k, v in times.items()}
        eng = next(iter(pipes[0]._engines.values()))
        out["c_job"] = {"regional_batch": B, "plain_batch": PB, "steps": args.steps, "rounds": args.rounds,
                        "launches_per_step": len(eng.calls)}
        out["c_first_call_s"] = round(first, 3)
        out["c_regional_s"] = [round(t, 5) for t in times["regional"]]
        out["c_plain_s"] = [round(t, 5) for t in times["plain"]]
        out["c_plain_again_s"] = [round(t, 5) for t in times["plain_again"]]
        out["c_regional_over_plain"] = round(med["regional"] / med["plain"], 4)
        out["c_plain_again_over_plain"] = round(med["plain_again"] / med["plain"], 4)
        both = times["plain"] + times["plain_again"]
        out["c_aa_spread"] = round((max(both) - min(both)) / statistics.median(both), 4)   # the plain job's own run-to-run range
        out["c_combine_share"] = round(args.steps * period * 1e-6 / med["plain"], 5)      # (a) x steps, as a fraction of the plain job
        out["c_images_per_s"] = round(B / med["regional"], 4)
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
