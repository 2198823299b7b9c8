#!/usr/bin/env python3
"""Cost of HyperTile (generate_image(..., hypertile=...), minsdtf_amd/hypertile.py) on one GPU, seeded synthetic SD1.5 weights:

  (i)  the msd_attention_windowed launch with 2 x 2 windows, batch 2, 8 heads, at the three windowed level shapes of a 1024x1024
       job - (S, d) = (16384, 40), (4096, 80), (1024, 160) - its per-launch period inside a replayed hipGraph, measured twice (A/A),
       next to msd_attention on the same operands unwindowed (the launch it replaces, 4x the FLOPs) and msd_attention on the windows
       gathered contiguously as batch 8 (the same FLOPs with no gather);
  (ii) a 512 -> 1024 hires job (25 + 15 steps) with hypertile={"tile": 512, "depth": 1} and without, ending in the latent, timed in
       alternation in this one process, and the plain hires job a second time (A/A): the run-to-run range the ratio is to be read
       against.

    python tools/hypertile_bench.py --out profiles/hypertile_bench.json
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

LEVELS = ((128, 40), (64, 80), (32, 160))   # (feature map side, head size) of a 1024x1024 job's levels 0 .. 2


def main(argv=None):
    from regions_bench import graph_period_us

    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--skip-job", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)

    import torch

    from minsdtf_amd import host, hypertile, ops
    from minsdtf_amd.stable_diffusion import StableDiffusion

    host.fit_torch_threads()
    dev = torch.device("cuda:0")
    out = {"metric": "hypertile", "i_levels": []}

    # (i) the launch at the three level shapes
    B, H, NW = 2, 8, 2
    for side, d in LEVELS:
        S, C = side * side, H * d
        wside = side // NW
        q = (torch.randn(B, S, C, device=dev) * (d ** -0.5 * 1.4426950408889634)).to(torch.bfloat16)
        k = torch.randn(B, S, C, device=dev).to(torch.bfloat16)
        v = torch.randn(B, S, C, device=dev).to(torch.bfloat16)
        vt = v.permute(0, 2, 1).contiguous()
        win = torch.from_numpy(hypertile.window_tokens(side, side, wside, wside)).to(dev)   # (4, S / 4)
        T = win.shape[1]
        qg, kg = (x[:, win].reshape(B * NW * NW, T, C).contiguous() for x in (q, k))
        vtg = v[:, win].reshape(B * NW * NW, T, C).permute(0, 2, 1).contiguous()
        o = torch.zeros(B, S, C, dtype=torch.bfloat16, device=dev)
        og = torch.zeros(B * NW * NW, T, C, dtype=torch.bfloat16, device=dev)
        ld = dict(q_ld=C, k_ld=C, o_ld=C)
        wd = ops.attention_windowed(q=q, k=k, vt=vt, out=o, batch=B, heads=H, head_dim=d, h=side, w=side, wh=wside, ww=wside, vt_ld=S, **ld)
        full = ops.attention(q=q, k=k, vt=vt, out=o, batch=B, heads=H, head_dim=d, s=S, t=S, vt_ld=S, scale=d ** -0.5, q_prescaled=True, **ld)
        cont = ops.attention(q=qg, k=kg, vt=vtg, out=og, batch=B * NW * NW, heads=H, head_dim=d, s=T, t=T, vt_ld=T, scale=d ** -0.5,
                             q_prescaled=True, **ld)
        n = 200 if S <= 1024 else 50 if S <= 4096 else 20
        p = {name: [graph_period_us(lambda st, c=c: c(st.cuda_stream), n=n) for _ in range(2)]   # (twice: A/A)
             for name, c in (("windowed", wd), ("attention_unwindowed", full), ("attention_gathered", cont))}
        best = {k_: min(v_) for k_, v_ in p.items()}
        spread = {k_: round((max(v_) - min(v_)) / min(v_), 4) for k_, v_ in p.items()}
        out["i_levels"].append({
            "s": S, "head_dim": d, "heads": H, "batch": B, "windows": [NW, NW], "window_tokens": T,
            "period_us": {k_: [round(x, 3) for x in v_] for k_, v_ in p.items()},
            "aa_spread": spread,
            "windowed_over_unwindowed": round(best["windowed"] / best["attention_unwindowed"], 3),
            "windowed_over_gathered": round(best["windowed"] / best["attention_gathered"], 3),
            # the one condition fixed in advance (checked at (16384, 40)): faster than the launch it replaces by more than the A/A spread
            "faster_than_unwindowed_beyond_aa": bool(max(p["windowed"]) < min(p["attention_unwindowed"]) * (1.0 - max(spread.values()))),
        })

    if not args.skip_job:
        rng = np.random.default_rng(0)
        ctx = rng.standard_normal((77, 768)).astype(np.float32)
        unc = rng.standard_normal((77, 768)).astype(np.float32)
        pipes = []
        for _ in range(3):   # one pipeline per timed job, so each keeps its two engines resident; one set of packed weights
            p = StableDiffusion(args.size, args.size, jit_compile=True, device=dev)
            if pipes:
                p._diffusion_model = pipes[0].diffusion_model
            else:
                p.diffusion_model.load_synthetic(seed=0)
            p.unconditional_context = unc
            pipes.append(p)
        kw = dict(num_steps=args.steps, unconditional_guidance_scale=7.5, seed=0, guidance_rescale=0.7, return_latent=True, batch_size=1,
                  hires=dict(scale=2))
        spec = dict(tile=args.size, depth=1)

        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        jobs = {
            "hypertile": lambda: pipes[0].generate_image(ctx, hypertile=spec, **kw),
            "plain": lambda: pipes[1].generate_image(ctx, **kw),
            "plain_again": lambda: pipes[2].generate_image(ctx, **kw),
        }
        first = timed(jobs["hypertile"])
        for fn in jobs.values():
            fn()   # warm: engines built, loops captured
        times = {k_: [] for k_ in jobs}
        for _ in range(args.rounds):
            for k_, fn in jobs.items():
                times[k_].append(timed(fn))
        med = {k_: statistics.median(v_) for k_, v_ in times.items()}
        run2 = int(args.steps * 0.6 + 0.5)
        out["ii_job"] = {"size": [args.size, 2 * args.size], "batch": 1, "steps": [args.steps, run2], "rounds": args.rounds,
                         "hypertile": spec, "windows": list(hypertile.parse(spec).key(2 * args.size, 2 * args.size))}
        out["ii_first_call_s"] = round(first, 3)
        for k_ in jobs:
            out[f"ii_{k_}_s"] = [round(t, 5) for t in times[k_]]
        out["ii_hypertile_over_plain"] = round(med["hypertile"] / med["plain"], 4)
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
