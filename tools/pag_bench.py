#!/usr/bin/env python3
"""Cost of perturbed-attention guidance (generate_image(..., pag=...), minsdtf_amd/pag.py) on one GPU, seeded synthetic SD1.5
weights:

  (a) the identity launch (msd_attention_identity; default: the rows of a 64 x 64-latent job's largest block, batch 2 x 320 channels x
      4096 keys, as the engine records it): its per-launch period inside a replayed hipGraph, next to the empty-kernel launch floor
      tools/launch_floor.py reports on the same box, and the bytes it moves per second;
  (b) the PAG job (batch B: 3 B UNet rows per step) against a regional job of R = 2 regions of the same batch - the same 3 B UNet
      rows, the same combine launch; what differs is the identity launches and the attention launches they shorten - both ending in
      the latent (the loops are what is compared), timed in alternation in this one process;
  (c) the regional job a second time (A/A): the run-to-run range (b) is to be read against.

    python tools/pag_bench.py --out profiles/pag_bench.json
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
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--scale", type=float, default=3.0)
    ap.add_argument("--layers", nargs="+", default=["mid"])
    ap.add_argument("--skip-job", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    B = args.batch

    floor, err = launch_floor_us()   # (first: a child process, before this one opens the GPU)
    import torch

    from minsdtf_amd import host, ops, pag, regions
    from minsdtf_amd.stable_diffusion import StableDiffusion

    host.fit_torch_threads()
    dev = torch.device("cuda:0")
    h = w = args.size // 8
    spec = pag.parse(dict(scale=args.scale, layers=args.layers))
    out = {"metric": "pag", "shape": {"size": args.size, "batch": B, "unet_rows": 3 * B, "layers": list(spec.key), "scale": spec.scale}}

    # (a) the launch at the first level's shape: S = h * w keys, 320 channels
    S, C = h * w, 320
    ld = (S + 7) // 8 * 8
    vt = torch.randn(B, C, ld, device=dev).to(torch.bfloat16)
    o = torch.zeros(B, S, C, dtype=torch.bfloat16, device=dev)
    call = ops.attention_identity(vt=vt, out=o, batch=B, channels=C, s=S, vt_ld=ld, o_ld=C)
    period = graph_period_us(lambda st: call(st.cuda_stream))
    out["a_shape"] = {"batch": B, "channels": C, "s": S}
    out["a_graph_period_us"] = round(period, 3)
    out["a_launch_floor_us"] = floor if floor is not None else {"error": err}
    if floor:
        out["a_period_over_floor"] = round(period / floor, 3)
    out["a_gbytes_per_s"] = round(2 * B * C * S * 2 / (period * 1e-6) / 1e9, 1)   # read + written

    if not args.skip_job:
        rng = np.random.default_rng(0)
        ctx = rng.standard_normal((77, 768)).astype(np.float32)
        unc = rng.standard_normal((77, 768)).astype(np.float32)
        job = dict(regions=[dict(prompt=rng.standard_normal((77, 768)).astype(np.float32), mask=m) for m in regions.boxes(h, w, 1, 2)])
        pipes = []
        for _ in range(3):   # one pipeline per timed job, so each keeps its engine resident; one set of packed weights
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
            "pag": lambda: pipes[0].generate_image(ctx, pag=spec, **kw),
            "regional": lambda: pipes[1].generate_image(ctx, regions=job, **kw),
            "regional_again": lambda: pipes[2].generate_image(ctx, regions=job, **kw),
        }
        first = timed(jobs["pag"])
        for fn in jobs.values():
            fn()   # warm: engines built, loops captured
        times = {k: [] for k in jobs}
        for _ in range(args.rounds):
            for k, fn in jobs.items():
                times[k].append(timed(fn))
        med = {k: statistics.median(v) for k, v in times.items()}
        eng = next(iter(pipes[0]._engines.values()))
        names = [c.name for c in eng.calls]
        out["b_job"] = {"batch": B, "steps": args.steps, "rounds": args.rounds, "launches_per_step": len(names),
                        "identity_launches_per_step": sum(n.endswith(".identity") for n in names),
                        "regional_launches_per_step": len(next(iter(pipes[1]._engines.values())).calls)}
        out["b_first_call_s"] = round(first, 3)
        out["b_pag_s"] = [round(t, 5) for t in times["pag"]]
        out["b_regional_s"] = [round(t, 5) for t in times["regional"]]
        out["c_regional_again_s"] = [round(t, 5) for t in times["regional_again"]]
        out["b_pag_over_regional"] = round(med["pag"] / med["regional"], 4)
        out["c_regional_again_over_regional"] = round(med["regional_again"] / med["regional"], 4)
        both = times["regional"] + times["regional_again"]
        out["c_aa_spread"] = round((max(both) - min(both)) / statistics.median(both), 4)   # the regional job's own run-to-run range
        out["b_images_per_s"] = round(B / med["pag"], 4)
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
