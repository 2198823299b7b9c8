#!/usr/bin/env python3
"""Cost of reference AdaIN (generate_image(..., reference_only={..., "adain": ...}), minsdtf_amd/reference.py) on one GPU, seeded
synthetic SD1.5 weights:

  (i)  the msd_reference_adain launch at (rows, hw, C) = (2, 64, 1280), (2, 256, 1280), (2, 1024, 1280) and (11, 1024, 1280) - the
       8 x 8, 16 x 16 and 32 x 32 levels of a 512x512 job at batch 1, and the 12-row cap - with mix 0.5 on every row: its
       per-launch period inside a replayed hipGraph, each measured twice (A/A), set against the two floors a launch cannot beat:
       the empty-kernel launch floor of tools/launch_floor.py, and the bytes it must move (rows + 1 rows read, rows written) at
       the HBM rate bench.py --full reports against (bench.HBM_PEAK_GBS).  The graph rewrites one buffer n times, so the operands
       are cache-resident, as a site tensor is behind the conv that produced it;
  (ii) a 512x512, 25-step, batch-1 job with adain="auto" plus all 16 attention blocks, the same job with adain off, and the
       plain job, all ending in the latent, timed in alternation in this one process, and the plain job a second time (A/A): the
       run-to-run range the ratios are to be read against.

    python tools/reference_adain_bench.py --out profiles/reference_adain_bench.json
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

SHAPES = ((2, 64, 1280), (2, 256, 1280), (2, 1024, 1280), (11, 1024, 1280))


def main(argv=None):
    from regions_bench import graph_period_us, launch_floor_us

    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip-job", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)

    floor, err = launch_floor_us()   # (first: a child process, before this one opens the GPU)
    import torch

    import bench
    from minsdtf_amd import host, ops
    from minsdtf_amd.stable_diffusion import StableDiffusion

    assert torch.cuda.is_available(), "reference_adain_bench.py measures on a GPU"
    host.fit_torch_threads()
    dev = torch.device("cuda:0")
    hbm = float(bench.HBM_PEAK_GBS)
    out = {"metric": "reference_adain", "launch_floor_us": floor, "launch_floor_error": err, "hbm_gbs": hbm, "i_launch": []}

    # (i) the launch
    for rows, hw, c in SHAPES:
        buf = torch.randn(rows + 1, hw, c, device=dev).to(torch.bfloat16)   # the engine's layout: the reference row last
        mix = torch.full((rows,), 0.5, dtype=torch.float32, device=dev)
        call = ops.reference_adain(x=buf, ref=buf[rows], mix=mix, rows=rows, hw=hw, c=c)
        p = [graph_period_us(lambda st: call(st.cuda_stream), n=200) for _ in range(2)]   # (twice: A/A)
        assert bool(torch.isfinite(buf.float()).all())
        nbytes = (2 * rows + 1) * hw * c * 2
        byte_floor = nbytes / (hbm * 1e9) * 1e6
        rec = {"rows": rows, "hw": hw, "c": c, "workgroups": rows * ((c + 63) // 64), "resident": hw <= ops.ADAIN_RESIDENT_HW,
               "period_us": [round(x, 3) for x in p], "aa_spread": round((max(p) - min(p)) / min(p), 4),
               "bytes": nbytes, "byte_floor_us": round(byte_floor, 3), "achieved_gbs": round(nbytes / (min(p) * 1e-6) / 1e9, 1)}
        if floor:
            rec["over_launch_floor"] = round(min(p) / floor, 3)
            rec["over_sum_of_floors"] = round(min(p) / (floor + byte_floor), 3)
        out["i_launch"].append(rec)

    if not args.skip_job:
        h = w = args.size // 8
        rng = np.random.default_rng(0)
        ctx = rng.standard_normal((77, 768)).astype(np.float32)
        unc = rng.standard_normal((77, 768)).astype(np.float32)
        z_ref = rng.standard_normal((1, h, w, 4)).astype(np.float32)
        pipes = []
        for _ in range(4):   # one pipeline per timed job, so each keeps its engine resident; one set of packed weights
            p = StableDiffusion(args.size, args.size, jit_compile=True, device=dev)
            if pipes:
                p._diffusion_model = pipes[0].diffusion_model
            else:
                p.diffusion_model.load_synthetic(seed=0)
            p.unconditional_context = unc
            pipes.append(p)
        kw = dict(num_steps=args.steps, unconditional_guidance_scale=7.5, seed=0, guidance_rescale=0.7, return_latent=True, batch_size=1)

        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        jobs = {
            "adain": lambda: pipes[0].generate_image(ctx, reference_only=dict(latent=z_ref, fidelity=0.5, adain="auto"), **kw),
            "adain_off": lambda: pipes[1].generate_image(ctx, reference_only=dict(latent=z_ref, fidelity=0.5), **kw),
            "plain": lambda: pipes[2].generate_image(ctx, **kw),
            "plain_again": lambda: pipes[3].generate_image(ctx, **kw),
        }
        first = timed(jobs["adain"])
        for fn in jobs.values():
            fn()   # warm: engines built, loops captured
        times = {k_: [] for k_ in jobs}
        for _ in range(args.rounds):
            for k_, fn in jobs.items():
                times[k_].append(timed(fn))
        med = {k_: statistics.median(v) for k_, v in times.items()}
        calls = {n: [c.name for c in next(iter(pipes[i]._engines.values())).calls] for i, n in enumerate(("adain", "adain_off", "plain"))}
        out["ii_job"] = {"size": args.size, "batch": 1, "steps": args.steps, "rounds": args.rounds,
                         "unet_rows": {"adain": 3, "adain_off": 3, "plain": 2},
                         "launches_per_step": {n: len(v) for n, v in calls.items()},
                         "adain_launches_per_step": sum(n.endswith(".adain") for n in calls["adain"])}
        out["ii_first_call_s"] = round(first, 3)
        for k_ in jobs:
            out[f"ii_{k_}_s"] = [round(t, 5) for t in times[k_]]
        out["ii_adain_over_adain_off"] = round(med["adain"] / med["adain_off"], 4)
        out["ii_adain_over_plain"] = round(med["adain"] / med["plain"], 4)
        out["ii_adain_off_over_plain"] = round(med["adain_off"] / med["plain"], 4)
        out["ii_us_per_adain_launch"] = round((med["adain"] - med["adain_off"]) * 1e6 / (args.steps * out["ii_job"]["adain_launches_per_step"]), 2)
        both = times["plain"] + times["plain_again"]
        out["ii_aa_spread"] = round((max(both) - min(both)) / statistics.median(both), 4)   # the plain job's own run-to-run range
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
