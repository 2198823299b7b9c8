#!/usr/bin/env python3
"""Cost of self-attention guidance (generate_image(..., sag=...), minsdtf_amd/sag.py) on one GPU, seeded synthetic SD1.5 weights:

  (a) the two launches a SAG step adds between its UNet passes - msdx_attention_colsum at the mid block's shape (batch B x 8 heads x
      d = 160 x (size / 64)^2 tokens) and msdx_sag_degrade on the B x size/8 x size/8 latent - each as its per-launch period inside a
      replayed hipGraph, next to the empty-kernel launch floor tools/launch_floor.py reports on the same box (colsum is two kernels
      behind the one entry: its period is to be read against twice the floor);
  (b) the SAG job (batch B: 2 B + B UNet rows per step, the B rows of the second pass DEPENDENT on the first) against a PAG job of
      the same 3 B rows in one pass and against the plain job of 2 B rows, all ending in the latent, timed in alternation in this
      one process;
  (c) every job a second time on a pipeline of its own (A/A): the run-to-run range (b) is to be read against.

    python tools/sag_bench.py --out profiles/sag_bench.json
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


def main(argv=None):
    from regions_bench import graph_period_us, launch_floor_us

    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--scale", type=float, default=0.75)
    ap.add_argument("--skip-job", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    B = args.batch

    floor, err = launch_floor_us()   # (first: a child process, before this one opens the GPU)
    import torch

    from minsdtf_amd import engine, host, ops, sag
    from minsdtf_amd.stable_diffusion import StableDiffusion

    host.fit_torch_threads()
    dev = torch.device("cuda:0")
    h = w = args.size // 8
    mh, mw = engine.unet_levels(h, w)[3]
    S, C = mh * mw, 1280
    spec = sag.parse(dict(scale=args.scale))
    out = {"metric": "sag", "shape": {"size": args.size, "batch": B, "unet_rows": 3 * B, "mid_tokens": S, "scale": spec.scale}}

    # (a) the two launches at the job's shapes
    q = (torch.randn(B, S, C, device=dev) * (2.0 / 160 ** 0.5)).to(torch.bfloat16)
    k = torch.randn(B, S, C, device=dev).to(torch.bfloat16)
    A = torch.zeros(B, S, device=dev)
    ws = torch.zeros(ops.colsum_workspace_floats(B, 8, S), device=dev)
    colsum = ops.attention_colsum(q=q, k=k, out=A, workspace=ws, batch=B, heads=8, head_dim=160, s=S, q_ld=C, k_ld=C)
    lat, eps, deg = (torch.randn(B, h, w, 4, device=dev) for _ in range(3))
    coef = torch.tensor([[0.8, 0.6, 0.0, 0.0]], device=dev)
    par = torch.from_numpy(sag.params(spec)).to(dev)
    step0 = torch.zeros(1, dtype=torch.int32, device=dev)
    degrade = ops.sag_degrade(latent=lat, eps=eps, coef=coef, coef_stride=4, step_ptr=step0, colsum=A, params=par, out=deg, batch=B, h=h, w=w,
                              mh=mh, mw=mw, num_steps=1)
    out["a_launch_floor_us"] = floor if floor is not None else {"error": err}
    for name, call in (("colsum", colsum), ("degrade", degrade)):
        period = graph_period_us(lambda st, c=call: c(st.cuda_stream))
        out[f"a_{name}_graph_period_us"] = round(period, 3)
        if floor:
            out[f"a_{name}_period_over_floor"] = round(period / floor, 3)

    if not args.skip_job:
        rng = np.random.default_rng(0)
        ctx = rng.standard_normal((77, 768)).astype(np.float32)
        unc = rng.standard_normal((77, 768)).astype(np.float32)
        kinds = {"sag": dict(sag=spec), "pag": dict(pag=dict(scale=3.0, layers="mid")), "plain": {}}
        pipes = {}
        for name in [k_ + s_ for k_ in kinds for s_ in ("", "_again")]:   # one pipeline per timed job: each keeps its engine resident
            p = StableDiffusion(args.size, args.size, jit_compile=True, device=dev)
            if pipes:
                p._diffusion_model = next(iter(pipes.values())).diffusion_model
            else:
                p.diffusion_model.load_synthetic(seed=0)
            p.unconditional_context = unc
            pipes[name] = p
        kw = dict(num_steps=args.steps, unconditional_guidance_scale=7.5, seed=0, guidance_rescale=0.7, return_latent=True, batch_size=B)

        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        jobs = {name: (lambda p=p, extra=kinds[name.replace("_again", "")]: p.generate_image(ctx, **extra, **kw)) for name, p in pipes.items()}
        first = timed(jobs["sag"])
        for fn in jobs.values():
            fn()   # warm: engines built, loops captured
        times = {k_: [] for k_ in jobs}
        for _ in range(args.rounds):
            for k_, fn in jobs.items():
                times[k_].append(timed(fn))
        med = {k_: statistics.median(v) for k_, v in times.items()}
        launches = {k_: len(next(iter(pipes[k_]._engines.values())).calls) for k_ in kinds}
        out["b_job"] = {"batch": B, "steps": args.steps, "rounds": args.rounds, "launches_per_step": launches}
        out["b_first_call_s"] = round(first, 3)
        for k_ in jobs:
            out[("c_" if k_.endswith("_again") else "b_") + k_ + "_s"] = [round(t, 5) for t in times[k_]]
        out["b_sag_over_pag"] = round(med["sag"] / med["pag"], 4)
        out["b_sag_over_plain"] = round(med["sag"] / med["plain"], 4)
        out["b_pag_over_plain"] = round(med["pag"] / med["plain"], 4)
        for k_ in kinds:
            both = times[k_] + times[k_ + "_again"]
            out[f"c_{k_}_again_over_{k_}"] = round(med[k_ + "_again"] / med[k_], 4)
            out[f"c_{k_}_aa_spread"] = round((max(both) - min(both)) / statistics.median(both), 4)
        out["b_images_per_s"] = round(B / med["sag"], 4)
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
