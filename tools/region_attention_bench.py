#!/usr/bin/env python3
"""Cost of regional prompting inside cross-attention (generate_image(..., regions={..., "mode": "attention"}), minsdtf_amd/regions.py)
on one GPU, seeded synthetic SD1.5 weights, R box regions (default: 512x512, 25 steps, batch 1, a 1 x 3 grid):

  (a) the msd_region_attention launch at the first level's shape (batch x 8 heads x 40 channels, S = h * w queries, 77 keys, the
      job's own level-0 plane): its per-launch period inside a replayed hipGraph, next to the empty-kernel launch floor
      tools/launch_floor.py reports on the same box and to the msd_attention launch it replaces (same q, region 0's K / V^T);
  (b) the attention-mode job, the latent-mode job of the same regions and the plain job, all ending in the latent (the loops are what
      is compared), timed in alternation in this one process;
  (c) the plain job a second time (A/A): the run-to-run range (b) is to be read against.  The claim to check: the attention-mode
      job is faster than the latent-mode job by more than that range.

Box masks are the favourable case: most workgroups keep one region.  With soft masks that are positive everywhere the launch is R
times a cross-attention; --soft times that case instead.

    python tools/region_attention_bench.py --out profiles/region_attention_bench.json
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
    ap.add_argument("--regions", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--soft", action="store_true", help="soft masks, positive everywhere, instead of boxes")
    ap.add_argument("--skip-job", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    B, R = args.batch, args.regions

    floor, err = launch_floor_us()   # (first: a child process, before this one opens the GPU)
    import torch

    from minsdtf_amd import engine, host, ops, regions
    from minsdtf_amd.stable_diffusion import StableDiffusion

    host.fit_torch_threads()
    dev = torch.device("cuda:0")
    h = w = args.size // 8
    rng = np.random.default_rng(0)
    masks = regions.boxes(h, w, 1, R)
    if args.soft:
        masks = [m + 0.25 for m in masks]
    prompts = [rng.standard_normal((77, 768)).astype(np.float32) for _ in range(R)]
    out = {"metric": "region_attention", "shape": {"size": args.size, "batch": B, "regions": R, "masks": "soft" if args.soft else "boxes",
                                                   "unet_rows": {"attention": 2 * B, "latent": (1 + R) * B, "plain": 2 * B}}}

    # (a) the launch at the first level's shape
    S, H, d, T = h * w, 8, 40, 77
    C, tp = H * d, 80
    res = regions.parse(dict(regions=[dict(prompt=p, mask=m) for p, m in zip(prompts, masks)], mode="attention"), args.size, args.size)
    plane = torch.from_numpy(res.level_weights(engine.unet_levels(h, w))[0].reshape(R, S)).to(dev)
    q = (torch.randn(B, S, C, device=dev) * (d ** -0.5 * 1.4426950408889634)).to(torch.bfloat16)
    k = torch.randn(R * B, T, C, device=dev).to(torch.bfloat16)
    vt = torch.zeros(R * B, C, tp, dtype=torch.bfloat16, device=dev)
    vt[:, :, :T] = torch.randn(R * B, C, T, device=dev).to(torch.bfloat16)
    o = torch.zeros(B, S, C, dtype=torch.bfloat16, device=dev)
    geo = dict(batch=B, heads=H, head_dim=d, s=S, t=T, q_ld=C, k_ld=C, vt_ld=tp, o_ld=C)
    ra = ops.region_attention(q=q, k=k, vt=vt, w=plane, out=o, regions=R, w_ld=S, **geo)
    at = ops.attention(q=q, k=k, vt=vt, out=o, scale=d ** -0.5, q_prescaled=True, **geo)
    p_ra = graph_period_us(lambda st: ra(st.cuda_stream))
    p_at = graph_period_us(lambda st: at(st.cuda_stream))
    out["a_shape"] = dict(geo, regions=R)
    out["a_region_attention_period_us"] = round(p_ra, 3)
    out["a_attention_period_us"] = round(p_at, 3)
    out["a_region_over_attention"] = round(p_ra / p_at, 3)
    out["a_launch_floor_us"] = floor if floor is not None else {"error": err}
    if floor:
        out["a_period_over_floor"] = round(p_ra / floor, 3)

    if not args.skip_job:
        ctx = rng.standard_normal((77, 768)).astype(np.float32)
        unc = rng.standard_normal((77, 768)).astype(np.float32)
        spec = [dict(prompt=p, mask=m) for p, m in zip(prompts, masks)]
        pipes = []
        for _ in range(4):   # one pipeline per timed job, so each keeps its engine resident; one set of packed weights
            p = StableDiffusion(args.size, args.size, jit_compile=True, device=dev)
            if pipes:
                p._diffusion_model = pipes[0].diffusion_model
            else:
                p.diffusion_model.load_synthetic(seed=0)
            p.unconditional_context = unc
            pipes.append(p)
        kw = dict(num_steps=args.steps, unconditional_guidance_scale=7.5, seed=0, guidance_rescale=0.7, return_latent=True, batch_size=B)

        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        jobs = {
            "attention": lambda: pipes[0].generate_image(ctx, regions=dict(regions=spec, mode="attention"), **kw),
            "latent": lambda: pipes[1].generate_image(ctx, regions=dict(regions=spec, mode="latent"), **kw),
            "plain": lambda: pipes[2].generate_image(ctx, **kw),
            "plain_again": lambda: pipes[3].generate_image(ctx, **kw),
        }
        first = timed(jobs["attention"])
        for fn in jobs.values():
            fn()   # warm: engines built, loops captured
        times = {k_: [] for k_ in jobs}
        for _ in range(args.rounds):
            for k_, fn in jobs.items():
                times[k_].append(timed(fn))
        med = {k_: statistics.median(v) for k_, v in times.items()}
        out["b_job"] = {"batch": B, "steps": args.steps, "rounds": args.rounds,
                        "launches_per_step": {n: len(next(iter(pipes[i]._engines.values())).calls) for i, n in enumerate(("attention", "latent", "plain"))}}
        out["b_first_call_s"] = round(first, 3)
        for k_ in ("attention", "latent", "plain"):
            out[f"b_{k_}_s"] = [round(t, 5) for t in times[k_]]
        out["c_plain_again_s"] = [round(t, 5) for t in times["plain_again"]]
        out["b_attention_over_latent"] = round(med["attention"] / med["latent"], 4)
        out["b_attention_over_plain"] = round(med["attention"] / med["plain"], 4)
        out["b_latent_over_plain"] = round(med["latent"] / med["plain"], 4)
        both = times["plain"] + times["plain_again"]
        out["c_aa_spread"] = round((max(both) - min(both)) / statistics.median(both), 4)   # the plain job's own run-to-run range
        out["b_attention_faster_than_latent_by_more_than_aa"] = bool(1.0 - med["attention"] / med["latent"] > out["c_aa_spread"])
        out["b_images_per_s"] = {k_: round(B / med[k_], 4) for k_ in ("attention", "latent", "plain")}
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
