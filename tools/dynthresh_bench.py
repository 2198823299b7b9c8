#!/usr/bin/env python3
"""Cost of dynamic thresholding (generate_image(..., dynamic_threshold=...), minsdtf_amd/dynthresh.py) on one GPU, seeded
synthetic SD1.5 weights:

  (a) the launch a step adds in front of its guidance / sampler step - msdt_dynamic_threshold at (B, h, w) = (1, 64, 64),
      (4, 64, 64), (1, 128, 128), measure "ad" at percentile 0.95 (the selection runs), at percentile 1 (one max reduction stands
      for it) and measure "std" (neither) - as its
      per-launch period inside a replayed hipGraph, next to the empty-kernel launch floor tools/launch_floor.py reports on the same
      box and next to the bytes it must move at 8 TB/s;
  (b) the same arithmetic as a composition of torch ops on the device (torch.quantile: a full sort and half a dozen elementwise
      launches; eager, since it could not read per-step scales from a device table inside a captured graph), timed with events
      around 50 calls; its result against the launch's, as a sanity check of what is being compared;
  (c) a 512x512, 25-step, batch-1 job with the feature against the plain job at the same guidance scale, timed in alternation in
      this one process, each job a second time on a pipeline of its own (A/A): the run-to-run range (c) is to be read against.

    python tools/dynthresh_bench.py --out profiles/dynthresh_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
SHAPES = [(1, 64, 64), (4, 64, 64), (1, 128, 128)]
HBM_BYTES_PER_US = 8e6   # 8 TB/s


def torch_composition(u, c, g, m, q):
    """dynthresh() with sep_feat_channels = True, measure "ad", startpoint "mean", phi = 1 on NHWC fp32 device tensors."""
    import torch

    B = u.shape[0]
    d = c - u
    cfg, mim = (u + g * d).reshape(B, -1, 4), (u + m * d).reshape(B, -1, 4)
    mean = cfg.mean(dim=1, keepdim=True)
    cc, mc = cfg - mean, mim - mim.mean(dim=1, keepdim=True)
    mim_ref = mc.abs().amax(dim=1, keepdim=True)
    cfg_ref = torch.quantile(cc.abs(), q, dim=1, keepdim=True)
    mx = torch.maximum(mim_ref, cfg_ref)
    return (torch.minimum(torch.maximum(cc, -mx), mx) / mx * mim_ref + mean).reshape(u.shape)


def main(argv=None):
    from regions_bench import graph_period_us, launch_floor_us

    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--guidance", type=float, default=14.0)
    ap.add_argument("--skip-job", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)

    floor, err = launch_floor_us()   # (first: a child process, before this one opens the GPU)
    import torch

    from minsdtf_amd import dynthresh, host, ops
    from minsdtf_amd.stable_diffusion import StableDiffusion

    host.fit_torch_threads()
    dev = torch.device("cuda:0")
    out = {"metric": "dynthresh", "a_launch_floor_us": floor if floor is not None else {"error": err}, "a_launch": [], "b_torch": []}
    g, m, q = 14.0, 7.0, 0.95
    for (B, h, w) in SHAPES:
        gen = torch.Generator(device="cpu").manual_seed(h * w + B)
        u = torch.randn(B, h, w, 4, generator=gen).to(dev)
        c = (u.cpu() + 0.3 * torch.randn(B, h, w, 4, generator=gen)).to(dev)
        eps = torch.cat([u, c]).reshape(2 * B, -1).contiguous()
        res = torch.zeros(B, h * w * 4, device=dev)
        scales = torch.tensor([[g, m]], dtype=torch.float32, device=dev)
        step0 = torch.zeros(1, dtype=torch.int32, device=dev)
        row = {"batch": B, "h": h, "w": w, "bytes_floor_us": round(3 * B * h * w * 16 / HBM_BYTES_PER_US, 3)}
        for tag, spec in (("ad", dict(percentile=q)), ("ad_p1", dict(percentile=1.0)), ("std", dict(measure="std"))):
            par = torch.from_numpy(dynthresh.params(spec, h * w)).to(dev)
            call = ops.dynamic_threshold(eps=eps, out=res, scales=scales, params=par, step_ptr=step0, batch=B, h=h, w=w, num_steps=1)
            periods = [graph_period_us(lambda st, c_=call: c_(st.cuda_stream)) for _ in range(2)]   # (twice: the A/A of the launch)
            row[f"{tag}_graph_period_us"] = [round(p, 3) for p in periods]
            if floor:
                row[f"{tag}_period_over_floor"] = round(min(periods) / floor, 3)
            if tag == "ad":
                mine = res.reshape(B, h, w, 4).clone()
        out["a_launch"].append(row)
        # (b) the torch route, eager
        ref = torch_composition(u, c, g, m, q)
        torch.cuda.synchronize()
        times = []
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(50):
                torch_composition(u, c, g, m, q)
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) * 1e3 / 50)
        out["b_torch"].append({"batch": B, "h": h, "w": w, "eager_period_us": [round(t, 2) for t in times],
                               "over_the_launch": round(min(times) / min(row["ad_graph_period_us"]), 2),
                               "max_abs_difference": float((ref - mine).abs().max())})

    if not args.skip_job:
        rng = np.random.default_rng(0)
        ctx = rng.standard_normal((77, 768)).astype(np.float32)
        unc = rng.standard_normal((77, 768)).astype(np.float32)
        kinds = {"dynthresh": dict(dynamic_threshold=dict(mimic_scale=7.0, percentile=0.95)), "plain": {}}
        pipes = {}
        for name in [k_ + s_ for k_ in kinds for s_ in ("", "_again")]:   # one pipeline per timed job: each keeps its engine resident
            p = StableDiffusion(args.size, args.size, jit_compile=True, device=dev)
            if pipes:
                p._diffusion_model = next(iter(pipes.values())).diffusion_model
            else:
                p.diffusion_model.load_synthetic(seed=0)
            p.unconditional_context = unc
            pipes[name] = p
        kw = dict(num_steps=args.steps, unconditional_guidance_scale=args.guidance, seed=0, guidance_rescale=0.0, return_latent=True,
                  batch_size=1)

        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        jobs = {name: (lambda p=p, extra=kinds[name.replace("_again", "")]: p.generate_image(ctx, **extra, **kw)) for name, p in pipes.items()}
        for fn in jobs.values():
            fn()   # warm: engines built, loops captured
        times = {k_: [] for k_ in jobs}
        for _ in range(args.rounds):
            for k_, fn in jobs.items():
                times[k_].append(timed(fn))
        med = {k_: statistics.median(v) for k_, v in times.items()}
        out["c_job"] = {"size": args.size, "batch": 1, "steps": args.steps, "rounds": args.rounds, "guidance": args.guidance,
                        "launches_per_step": {k_: len(next(iter(pipes[k_]._engines.values())).calls) for k_ in kinds}}
        for k_ in jobs:
            out["c_" + k_ + "_s"] = [round(t, 5) for t in times[k_]]
        out["c_dynthresh_over_plain"] = round(med["dynthresh"] / med["plain"], 4)
        for k_ in kinds:
            both = times[k_] + times[k_ + "_again"]
            out[f"c_{k_}_again_over_{k_}"] = round(med[k_ + "_again"] / med[k_], 4)
            out[f"c_{k_}_aa_spread"] = round((max(both) - min(both)) / statistics.median(both), 4)
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
