#!/usr/bin/env python3
"""Cost of T2I-Adapters (generate_image(..., t2i_adapter=...), minsdtf_amd/t2iadapter.py) on one GPU, seeded synthetic weights.  Every
period is taken inside a replayed hipGraph; every series is measured twice in alternation (A/A).

  (a) the launch floor (tools/launch_floor.py, a child process); msda_feature_add at the four site shapes of a 512x512 job, rows = 2 and
      8, 1 and 3 units, against the floor plus its bytes at 8 TB/s;
  (b) the adapter's 31-launch plan at 512x512: its replayed graph against 31 launch floors plus its weight bytes at 8 TB/s;
  (c) a 512x512, 25-step, batch-1 job: plain, with one adapter (a new picture each call, and the same picture repeated) and the plain
      ControlNet job, each with an A/A twin;
  (d) with --parent DIR (a built checkout of the parent commit): bench.py there and here in alternation, fresh processes.

    python tools/t2i_adapter_bench.py --out profiles/t2i_adapter_bench.json
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
HBM_BYTES_PER_S = 8.0e12


def main(argv=None):
    from regions_bench import graph_period_us, launch_floor_us
    from vision_bench import bench_ab

    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip-job", action="store_true")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: bench.py there and here in alternation")
    ap.add_argument("--bench-steps", type=int, default=10)
    ap.add_argument("--bench-warmup", type=int, default=2)
    ap.add_argument("--bench-rounds", type=int, default=3)
    ap.add_argument("--box", default=None, help="the name of the machine, recorded as it is")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)

    out = {"metric": "t2i_adapter", "size": args.size, "box": args.box}

    def save():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(json.dumps(out, indent=1) + "\n")

    if args.parent:   # (first: child processes, before this one opens the GPU)
        out["d_bench"] = bench_ab(args.parent, args.bench_steps, args.bench_warmup, args.bench_rounds)
        out["d_bench_images_per_s"] = {k: [r.get("value") for r in v] for k, v in out["d_bench"].items()}
        print(json.dumps(out["d_bench_images_per_s"]), flush=True)
    else:
        out["d_bench"] = "not measured (no --parent checkout given)"
    floor, err = launch_floor_us()
    import torch

    from minsdtf_amd import engine, host, ops
    from minsdtf_amd import weights as wtab
    from minsdtf_amd.models import T2IAdapter
    from minsdtf_amd.stable_diffusion import StableDiffusion

    host.fit_torch_threads()
    dev = torch.device("cuda:0")
    out["box"] = args.box or torch.cuda.get_device_name(0)
    out["a_launch_floor_us"] = floor if floor is not None else {"error": err}
    BF = torch.bfloat16
    h = w = args.size // 8

    # ---- (a) the add at the four site shapes
    out["a_feature_add"] = {}
    for site, ((hl, wl), ch) in enumerate(zip(engine.unet_levels(h, w), wtab.UNET_CH)):
        n = hl * wl * ch
        for rows in (2, 8):
            for U in (1, 3):
                x = torch.randn(rows, n, device=dev).to(BF)
                feats = [torch.randn(n, device=dev).to(BF) for _ in range(U)]
                sc = torch.full((1, U, 4), 1.0 / 64, dtype=torch.float32, device=dev)
                call = ops.feature_add(x=x, feats=feats, scales=sc, rows=rows, n=n, site=site, num_steps=1)
                nbytes = (2 * rows + U) * n * 2
                rec = {"site": site, "n": n, "rows": rows, "units": U, "workgroups": (n + 2047) // 2048, "bytes": nbytes,
                       "us": round(graph_period_us(lambda st, c=call: c(st.cuda_stream)), 3),
                       "again_us": round(graph_period_us(lambda st, c=call: c(st.cuda_stream)), 3),
                       "bytes_at_8TBs_us": round(nbytes / HBM_BYTES_PER_S * 1e6, 3)}
                if floor is not None:
                    rec["floor_plus_bytes_us"] = round(floor + nbytes / HBM_BYTES_PER_S * 1e6, 3)
                    rec["over_floor_plus_bytes"] = round(rec["us"] / rec["floor_plus_bytes_us"], 3)
                out["a_feature_add"][f"site{site}_rows{rows}_units{U}"] = rec
                print(json.dumps(rec), flush=True)
    save()

    # ---- (b) the adapter's plan
    ad = T2IAdapter.synthetic(7, 3, device=dev)
    ad.compile(jit_compile=True)
    rng = np.random.default_rng(0)
    ad.features(rng.random((1, args.size, args.size, 3)).astype(np.float32))
    bp = ad._plans[(args.size, args.size)]
    series = {"adapter": [], "adapter_again": []}
    for _ in range(args.rounds):
        for k in series:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _i in range(20):
                bp.graph.replay()
            e1.record()
            torch.cuda.synchronize()
            series[k].append(e0.elapsed_time(e1) * 1e3 / 20)
    launches = len(bp.plan.calls)
    wbytes = sum(int(t.numel()) * t.element_size() for t in ad._W.values() if isinstance(t, torch.Tensor))
    med = {k: statistics.median(v) for k, v in series.items()}
    both = series["adapter"] + series["adapter_again"]
    out["b_adapter"] = {"launches": launches, "weight_bytes": wbytes, "rounds": args.rounds, "replays_per_sample": 20,
                        "adapter_us": [round(v, 1) for v in series["adapter"]], "adapter_again_us": [round(v, 1) for v in series["adapter_again"]],
                        "median_us": round(med["adapter"], 1), "aa_ratio": round(med["adapter_again"] / med["adapter"], 4),
                        "aa_spread": round((max(both) - min(both)) / statistics.median(both), 4),
                        "weights_at_8TBs_us": round(wbytes / HBM_BYTES_PER_S * 1e6, 1),
                        "note": f"back-to-back replays re-read the {wbytes / 1e6:.0f} MB of weights from the caches where they fit: a lower bound of a cold call"}
    if floor is not None:
        fl = floor * launches + wbytes / HBM_BYTES_PER_S * 1e6
        out["b_adapter"].update(floor_us=round(fl, 1), over_floor=round(med["adapter"] / fl, 3))
    per = {}
    for c in bp.plan.calls:
        per[c.name] = round(graph_period_us(lambda st, c_=c: c_(st.cuda_stream), n=50), 2)
    out["b_launches_hot_weights_us"] = per
    print(json.dumps(out["b_adapter"]), flush=True)
    save()

    # ---- (c) the jobs
    if not args.skip_job:
        ctx, unc = (rng.standard_normal((77, 768)).astype(np.float32) for _ in range(2))
        img = rng.integers(0, 256, (args.size, args.size, 3)).astype(np.float32)
        pic = rng.integers(0, 256, (args.size, args.size, 3)).astype(np.uint8)
        kinds = ("plain", "adapter_repeated", "adapter_new_picture", "controlnet")
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
        kw = dict(num_steps=args.steps, unconditional_guidance_scale=7.5, seed=0, guidance_rescale=0.7, return_latent=True, batch_size=1)

        def job(name):
            p, kind = pipes[name], name.replace("_again", "")
            if kind == "plain":
                return lambda: p.generate_image(ctx, **kw)
            if kind == "controlnet":
                return lambda: p.generate_image(ctx, control_net_image=img, **kw)
            if kind == "adapter_repeated":
                return lambda: p.generate_image(ctx, t2i_adapter=dict(image=pic, model=ad), **kw)
            return lambda: p.generate_image(ctx, t2i_adapter=dict(image=rng.integers(0, 256, (args.size, args.size, 3)).astype(np.uint8), model=ad), **kw)

        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        jobs = {name: job(name) for name in pipes}
        for fn in jobs.values():   # warm: engines built, loops captured
            fn()
        times = {k_: [] for k_ in jobs}
        for _ in range(args.rounds):
            for k_, fn in jobs.items():
                times[k_].append(timed(fn))
        med = {k_: statistics.median(v) for k_, v in times.items()}
        rec = {"size": args.size, "batch": 1, "steps": args.steps, "rounds": args.rounds,
               "launches_per_step": {k_: len(next(iter(pipes[k_]._engines.values())).calls) for k_ in kinds}}
        for k_ in jobs:
            rec[k_ + "_s"] = [round(t, 5) for t in times[k_]]
        for k_ in kinds:
            both = times[k_] + times[k_ + "_again"]
            rec[f"{k_}_median_s"] = round(med[k_], 5)
            rec[f"{k_}_again_over_{k_}"] = round(med[k_ + "_again"] / med[k_], 4)
            rec[f"{k_}_aa_spread"] = round((max(both) - min(both)) / statistics.median(both), 4)
        rec["adapter_repeated_minus_plain_ms_per_step"] = round((med["adapter_repeated"] - med["plain"]) * 1e3 / args.steps, 4)
        rec["adapter_new_picture_minus_repeated_ms"] = round((med["adapter_new_picture"] - med["adapter_repeated"]) * 1e3, 3)
        rec["adapter_repeated_over_plain"] = round(med["adapter_repeated"] / med["plain"], 4)
        rec["controlnet_over_plain"] = round(med["controlnet"] / med["plain"], 4)
        rec["adapter_repeated_over_controlnet"] = round(med["adapter_repeated"] / med["controlnet"], 4)
        if floor is not None:
            rec["four_launch_floors_per_step_ms"] = round(4 * floor * 1e-3, 4)
        out["c_job"] = rec
    else:
        out["c_job"] = "not measured (--skip-job)"
    print(json.dumps(out), flush=True)
    save()


if __name__ == "__main__":
    main()
