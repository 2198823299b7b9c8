#!/usr/bin/env python3
"""Cost of ControlNet units (generate_image(..., control_net_image=img, control=...), minsdtf_amd/control.py) on one GPU, seeded
synthetic SD1.5 weights:

  (a) the ONE launch a UNet pass adds - msdc_control_combine over the 13 skip shapes of a 512x512 batch-1 job (2 rows, 1 of them
      unconditional) for N = 1, 2, 3 units - as its per-launch period inside a replayed hipGraph, each measured twice (A/A), next
      to the empty-kernel launch floor tools/launch_floor.py reports on the same box and next to the bytes it must move at 8 TB/s
      (per element and row: 2 read + 2 written + 4 N read);
  (b) 512x512, 25-step, batch-1 jobs, timed in alternation in this one process, each a second time on a pipeline of its own (A/A):
      the plain ControlNet job (control=None: the plans of the commit before the option, tools/plan_digest.py), the all-ones job
      (control={}: the same arithmetic, the 13 zero convs unfused and the one launch added) and a job with two units (a second
      ControlNet and HintNet); the ratios all-ones / plain, two units / plain and two units / all-ones.

    python tools/control_units_bench.py --out profiles/control_units_bench.json
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
HBM_BYTES_PER_US = 8e6   # 8 TB/s
LEVEL_OF_TAP = (0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3, 3)


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

    from minsdtf_amd import engine, host, ops
    from minsdtf_amd import weights as wtab
    from minsdtf_amd.models import ControlNet, HintNet
    from minsdtf_amd.stable_diffusion import StableDiffusion

    host.fit_torch_threads()
    dev = torch.device("cuda:0")
    out = {"metric": "control_units", "a_launch_floor_us": floor if floor is not None else {"error": err}, "a_launch": []}
    h = w = args.size // 8
    levels = engine.unet_levels(h, w)
    counts = [levels[lv][0] * levels[lv][1] * ch for lv, ch in zip(LEVEL_OF_TAP, tuple(wtab.UNET_SKIP_CH) + (1280,))]
    rows = 2
    gen = torch.Generator(device="cpu").manual_seed(0)
    skips = [torch.randn(rows, n, generator=gen).to(torch.bfloat16).to(dev) for n in counts]
    resid = [[torch.randn(rows, n, generator=gen).to(dev) for n in counts] for _ in range(3)]
    step0 = torch.zeros(1, dtype=torch.int32, device=dev)
    for N in (1, 2, 3):
        scales = torch.full((1, N, 13, 2), 0.75, dtype=torch.float32, device=dev)
        call = ops.control_combine(skips=skips, resid=resid[:N], counts=counts, scales=scales, step_ptr=step0, rows=rows, rows_u=1, num_steps=1)
        periods = [graph_period_us(lambda st, c_=call: c_(st.cuda_stream)) for _ in range(2)]   # (twice: the A/A of the launch)
        nbytes = rows * sum(counts) * (2 + 2 + 4 * N)
        row = {"units": N, "rows": rows, "elements_per_row": sum(counts), "workgroups": rows * ops.control_chunk_prefix(counts)[-1], "bytes": nbytes,
               "bytes_floor_us": round(nbytes / HBM_BYTES_PER_US, 3), "graph_period_us": [round(p, 3) for p in periods],
               "bytes_per_us": round(nbytes / min(periods)), "aa_ratio": round(max(periods) / min(periods), 4)}
        if floor:
            row["period_over_floor_plus_bytes"] = round(min(periods) / (floor + nbytes / HBM_BYTES_PER_US), 3)
        out["a_launch"].append(row)

    if not args.skip_job:
        rng = np.random.default_rng(0)
        ctx = rng.standard_normal((77, 768)).astype(np.float32)
        unc = rng.standard_normal((77, 768)).astype(np.float32)
        img, img2 = (rng.integers(0, 256, (args.size, args.size, 3)).astype(np.float32) for _ in range(2))
        cn1, hn1 = ControlNet(args.size, args.size, device=dev), HintNet(args.size, args.size, device=dev)
        cn1.load_synthetic(seed=1)
        hn1.load_synthetic(seed=1)
        kinds = {"plain": {}, "ones": dict(control={}), "two_units": dict(control=[dict(weight=1.0, mode="control"),
                                                                                  dict(image=img2, models=(cn1, hn1), weight=0.7, start=0.25)])}
        pipes = {}
        for name in [k_ + s_ for k_ in kinds for s_ in ("", "_again")]:   # one pipeline per timed job: each keeps its engine resident
            p = StableDiffusion(args.size, args.size, jit_compile=True, device=dev, controlnet_path="synthetic")
            if pipes:
                first = next(iter(pipes.values()))
                p._diffusion_model, p._control_net, p._hint_net = first.diffusion_model, first.control_net, first.hint_net
            else:
                p.diffusion_model.load_synthetic(seed=0)
                p.control_net.load_synthetic(seed=0)
                p.hint_net.load_synthetic(seed=0)
            p.unconditional_context = unc
            pipes[name] = p
        kw = dict(num_steps=args.steps, unconditional_guidance_scale=7.5, seed=0, guidance_rescale=0.7, return_latent=True, batch_size=1,
                  control_net_image=img)

        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        jobs = {name: (lambda p=p, extra=kinds[name.replace("_again", "")]: p.generate_image(ctx, **extra, **kw)) for name, p in pipes.items()}
        first = {name: fn() for name, fn in jobs.items()}   # warm: engines built, loops captured
        times = {k_: [] for k_ in jobs}
        for _ in range(args.rounds):
            for k_, fn in jobs.items():
                times[k_].append(timed(fn))
        med = {k_: statistics.median(v) for k_, v in times.items()}
        out["b_job"] = {"size": args.size, "batch": 1, "steps": args.steps, "rounds": args.rounds,
                        "launches_per_step": {k_: len(next(iter(pipes[k_]._engines.values())).calls) for k_ in kinds},
                        "ones_equals_plain_bit_for_bit": bool(np.array_equal(first["ones"], first["plain"]))}
        for k_ in jobs:
            out["b_" + k_ + "_s"] = [round(t, 5) for t in times[k_]]
        out["b_ones_over_plain"] = round(med["ones"] / med["plain"], 4)
        out["b_two_units_over_plain"] = round(med["two_units"] / med["plain"], 4)
        out["b_two_units_over_ones"] = round(med["two_units"] / med["ones"], 4)
        out["b_ones_minus_plain_ms_per_step"] = round((med["ones"] - med["plain"]) * 1e3 / args.steps, 4)
        for k_ in kinds:
            both = times[k_] + times[k_ + "_again"]
            out[f"b_{k_}_again_over_{k_}"] = round(med[k_ + "_again"] / med[k_], 4)
            out[f"b_{k_}_aa_spread"] = round((max(both) - min(both)) / statistics.median(both), 4)
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
