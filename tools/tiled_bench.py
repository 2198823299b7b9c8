#!/usr/bin/env python3
"""Cost of tiled diffusion (generate_image(..., tiled=...), minsdtf_amd/tiled.py) on one GPU, seeded synthetic SD1.5 weights:

  (a) the consensus launch (msd_tile_consensus; default: the views of a 512x1024 canvas at the 512-px tile, stride 256: a
      64 x 128 latent under 1 x 3 views): its per-launch period inside a replayed hipGraph, next to the empty-kernel launch
      floor tools/launch_floor.py reports on the same box;
  (b) the same hand-off composed from torch ops (per view a weighted add into an accumulator, one division, per view a copy
      back): its period inside a replayed graph and its number of kernel launches - both forms measured in this one process;
  (c) the tiled job against the plain job of the same engine batch and steps (both end in the latent: the loops are what is
      compared), the plain job twice (A/A), the three timed in alternation in this one process.  The tiled job should cost the
      plain job plus its consensus launches: tiled / plain is to be read against the A/A spread and (a) x steps.

    python tools/tiled_bench.py --out profiles/tiled_bench.json
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
    ap.add_argument("--tile", type=int, default=512)
    ap.add_argument("--size", type=int, nargs=2, default=[512, 1024])
    ap.add_argument("--stride", type=int, default=None)
    ap.add_argument("--blend", default="uniform")
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip-job", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)

    floor, err = launch_floor_us()   # (first: a child process, before this one opens the GPU)
    import torch

    from minsdtf_amd import host, ops, tiled
    from minsdtf_amd.stable_diffusion import StableDiffusion

    host.fit_torch_threads()
    dev = torch.device("cuda:0")
    spec = dict(size=tuple(args.size), stride=args.stride, blend=args.blend)
    geo = tiled.parse(spec, args.tile, args.tile)
    V = geo.views
    out = {"metric": "tiled", "geometry": {"tile": args.tile, "canvas": list(args.size), "ys": list(geo.ys), "xs": list(geo.xs), "views": V,
                                           "blend": geo.blend}}

    # (a) the launch, (b) the torch composition of it
    tiles = torch.randn(V, geo.th, geo.tw, 4, device=dev)
    canvas = torch.zeros(1, geo.H, geo.W, 4, device=dev)
    wy, wx = torch.from_numpy(geo.wy).to(dev), torch.from_numpy(geo.wx).to(dev)
    call = ops.tile_consensus(tiles=tiles, canvas=canvas, wy=wy, wx=wx, ys=geo.ys, xs=geo.xs, th=geo.th, tw=geo.tw, H=geo.H, W=geo.W, batch=1)
    w2 = (wy[:, None] * wx[None, :])[:, :, None]
    wsum = torch.zeros(geo.H, geo.W, 1, device=dev)
    for (y, x) in geo.offsets():
        wsum[y:y + geo.th, x:x + geo.tw] += w2
    acc = torch.zeros(geo.H, geo.W, 4, device=dev)
    launches = [0]

    def torch_route(_stream):
        acc.zero_()
        for v, (y, x) in enumerate(geo.offsets()):
            acc[y:y + geo.th, x:x + geo.tw].addcmul_(tiles[v], w2)
        torch.div(acc, wsum, out=canvas[0])
        for v, (y, x) in enumerate(geo.offsets()):
            tiles[v].copy_(canvas[0, y:y + geo.th, x:x + geo.tw])
        launches[0] = 2 + 2 * V

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
        pipes = []
        for _ in range(3):   # one pipeline per timed job, so each keeps its engine resident; one set of packed weights
            p = StableDiffusion(args.tile, args.tile, jit_compile=True, device=dev)
            if pipes:
                p._diffusion_model = pipes[0].diffusion_model
            else:
                p.diffusion_model.load_synthetic(seed=0)
            p.unconditional_context = unc
            pipes.append(p)
        kw = dict(num_steps=args.steps, unconditional_guidance_scale=7.5, seed=0, guidance_rescale=0.7, return_latent=True)

        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        jobs = {
            "tiled": lambda: pipes[0].generate_image(ctx, batch_size=1, tiled=spec, **kw),
            "plain": lambda: pipes[1].generate_image(ctx, batch_size=V, **kw),
            "plain_again": lambda: pipes[2].generate_image(ctx, batch_size=V, **kw),
        }
        first = timed(jobs["tiled"])
        for fn in jobs.values():
            fn()   # warm: engines built, loops captured
        times = {k: [] for k in jobs}
        for _ in range(args.rounds):
            for k, fn in jobs.items():
                times[k].append(timed(fn))
        med = {k: statistics.median(v) for k, v in times.items()}
        eng = next(iter(pipes[0]._engines.values()))
        out["c_job"] = {"engine_batch": V, "steps": args.steps, "rounds": args.rounds, "launches_per_step": len(eng.calls)}
        out["c_first_call_s"] = round(first, 3)
        out["c_tiled_s"] = [round(t, 5) for t in times["tiled"]]
        out["c_plain_s"] = [round(t, 5) for t in times["plain"]]
        out["c_plain_again_s"] = [round(t, 5) for t in times["plain_again"]]
        out["c_tiled_over_plain"] = round(med["tiled"] / med["plain"], 4)
        out["c_plain_again_over_plain"] = round(med["plain_again"] / med["plain"], 4)
        both = times["plain"] + times["plain_again"]
        out["c_aa_spread"] = round((max(both) - min(both)) / statistics.median(both), 4)   # the plain job's own run-to-run range
        out["c_consensus_share"] = round(args.steps * period * 1e-6 / med["plain"], 5)    # (a) x steps, as a fraction of the plain job
        out["c_canvases_per_s"] = round(1.0 / med["tiled"], 4)
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
