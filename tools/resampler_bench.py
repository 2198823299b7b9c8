#!/usr/bin/env python3
"""Cost of the IP-Adapter "plus" Resampler (models.IPResampler, minsdtf_amd/resampler.py) on one GPU, seeded synthetic weights.  Every
period is taken inside a replayed hipGraph; every series is measured twice in alternation (A/A).

  (a) the launch floor (tools/launch_floor.py, a child process); msdr_perceiver_attention at (batch 1 and 2, 12 heads, n = 16, t_x = 257)
      against it, and against msd_attention on the same keys gathered into one contiguous K and one V^T - with the four gather copies
      in the graph and without them;
  (b) the depth-4 resampler at batch 1: its replayed graph against launch count x launch floor + weight bytes / 8 TB/s, and every launch
      of one layer alone in a graph of its own;
  (c) a plus job from a picture (512x512, 25 steps, batch 1) on its first and its repeated call, next to the same job with tokens=;
  (d) with --parent DIR (a built checkout of the parent commit): bench.py there and here in alternation, fresh processes.

    python tools/resampler_bench.py --out profiles/ip_resampler_bench.json
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
LOG2E = 1.4426950408889634


def main(argv=None):
    from regions_bench import graph_period_us, launch_floor_us
    from vision_bench import bench_ab

    ap = argparse.ArgumentParser()
    ap.add_argument("--depth", type=int, default=4)
    ap.add_argument("--layers", type=int, default=32, help="layers of the vision tower of (c)")
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip-job", action="store_true")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: bench.py there and here in alternation")
    ap.add_argument("--bench-steps", type=int, default=10)
    ap.add_argument("--bench-warmup", type=int, default=2)
    ap.add_argument("--bench-rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)

    out = {"metric": "ip_resampler", "depth": args.depth}

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
    from minsdtf_amd.models import ClipVisionEncoder, IPAdapter, IPResampler
    from minsdtf_amd.stable_diffusion import StableDiffusion

    host.fit_torch_threads()
    dev = torch.device("cuda:0")
    out["a_launch_floor_us"] = floor if floor is not None else {"error": err}
    BF = torch.bfloat16

    # ---- (a) the kernel against the launch floor and against msd_attention on gathered keys
    H, n, t, C = 12, 16, 257, 768
    tp, T = 264, 257 + 16
    Tp = (T + 7) // 8 * 8
    out["a_attention"] = {}
    for B in (1, 2):
        g = torch.Generator().manual_seed(B)
        q, kl = (torch.randn(B, n, C, generator=g).to(BF).to(dev) for _ in range(2))
        kx = torch.randn(B, t, C, generator=g).to(BF).to(dev)
        vtx = torch.zeros(B, C, tp, dtype=BF, device=dev)
        vtx[:, :, :t] = torch.randn(B, C, t, generator=g).to(BF).to(dev)
        vtl = torch.randn(B, C, n, generator=g).to(BF).to(dev)
        o1, o2 = (torch.zeros(B, n, C, dtype=BF, device=dev) for _ in range(2))
        kcat, vtcat = torch.zeros(B, T, C, dtype=BF, device=dev), torch.zeros(B, C, Tp, dtype=BF, device=dev)
        pa = ops.perceiver_attention(q=q, k_x=kx, vt_x=vtx, k_l=kl, vt_l=vtl, out=o1, batch=B, heads=H, n=n, t_x=t, q_ld=C, kx_ld=C, vtx_ld=tp,
                                     kl_ld=C, vtl_ld=n, o_ld=C, scale=64 ** -0.5 * LOG2E)

        def gather():
            kcat[:, :t].copy_(kx)
            kcat[:, t:].copy_(kl)
            vtcat[:, :, :t].copy_(vtx[:, :, :t])
            vtcat[:, :, t:T].copy_(vtl)

        rec = {"batch": B, "workgroups": B * H}
        rec["perceiver_us"] = round(graph_period_us(lambda st: pa(st.cuda_stream)), 3)
        try:
            at = ops.attention(q=q, k=kcat, vt=vtcat, out=o2, batch=B, heads=H, head_dim=64, s=n, t=T, q_ld=C, k_ld=C, vt_ld=Tp, o_ld=C,
                               scale=64 ** -0.5)
            gather()
            rec["msd_attention_us"] = round(graph_period_us(lambda st: at(st.cuda_stream)), 3)

            def composed(st):
                with torch.cuda.stream(st):
                    gather()
                at(st.cuda_stream)

            rec["msd_attention_with_gather_us"] = round(graph_period_us(composed), 3)
            rec["msd_attention_again_us"] = round(graph_period_us(lambda st: at(st.cuda_stream)), 3)
            pa(torch.cuda.current_stream().cuda_stream)
            at(torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            rec["max_abs_difference_of_the_two_results"] = float((o1.float() - o2.float()).abs().max())
        except Exception as e:   # noqa: BLE001 - (the composition is the comparison, not the product: its failure is a result)
            rec["msd_attention_error"] = f"{type(e).__name__}: {e}"[:300]
        rec["perceiver_again_us"] = round(graph_period_us(lambda st: pa(st.cuda_stream)), 3)
        rec["aa_ratio"] = round(rec["perceiver_again_us"] / rec["perceiver_us"], 4)
        if floor is not None:
            rec["perceiver_over_launch_floor"] = round(rec["perceiver_us"] / floor, 2)
        out["a_attention"][f"batch{B}"] = rec
        print(json.dumps(rec), flush=True)
    save()

    # ---- (b) the resampler at batch 1
    rs = IPResampler(depth=args.depth, device=dev)
    rs.load_synthetic(seed=1)
    rs.compile(jit_compile=True)
    hidden = (1.2 * np.random.default_rng(0).standard_normal((1, 257, 1280))).astype(np.float32)
    rs.predict_on_batch(hidden)
    bp = rs._bound((1,), None)
    series = {"resampler": [], "resampler_again": []}
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
    assert launches == engine.ip_resampler_launches(args.depth, 1)
    wbytes = sum(int(w.numel()) * w.element_size() for w in rs._W.values() if isinstance(w, torch.Tensor))
    med = {k: statistics.median(v) for k, v in series.items()}
    both = series["resampler"] + series["resampler_again"]
    out["b_resampler"] = {"batch": 1, "launches": launches, "weight_bytes": wbytes, "rounds": args.rounds, "replays_per_sample": 20,
                          "resampler_us": [round(x, 1) for x in series["resampler"]], "resampler_again_us": [round(x, 1) for x in series["resampler_again"]],
                          "median_us": round(med["resampler"], 1), "aa_ratio": round(med["resampler_again"] / med["resampler"], 4),
                          "aa_spread": round((max(both) - min(both)) / statistics.median(both), 4),
                          "weights_at_8TBs_us": round(wbytes / HBM_BYTES_PER_S * 1e6, 1),
                          "note": f"back-to-back replays re-read the {wbytes / 1e6:.0f} MB of weights from the caches where they fit: a lower bound of a cold call"}
    if floor is not None:
        fl = floor * launches + wbytes / HBM_BYTES_PER_S * 1e6
        out["b_resampler"].update(floor_us=round(fl, 1), over_floor=round(med["resampler"] / fl, 3))
    print(json.dumps(out["b_resampler"]), flush=True)
    share = {}
    first = next(i for i, c in enumerate(bp.plan.calls) if c.name.startswith("layers.0."))
    for i in list(range(0, first)) + list(range(first, first + engine.RESAMPLER_LAYER_LAUNCHES)) + list(range(launches - 3, launches)):
        c = bp.plan.calls[i]
        share[c.name] = {"us": round(graph_period_us(lambda st, c_=c: c_(st.cuda_stream), n=50), 2),
                         "again_us": round(graph_period_us(lambda st, c_=c: c_(st.cuda_stream), n=50), 2)}
    out["b_launches_hot_weights"] = share
    out["b_layer_sum_hot_us"] = round(sum(v["us"] for k, v in share.items() if k.startswith("layers.0.")), 1)
    print(json.dumps(share), flush=True)
    save()

    # ---- (c) the job from a picture
    if not args.skip_job:
        rng = np.random.default_rng(0)
        ctx, unc = (rng.standard_normal((77, 768)).astype(np.float32) for _ in range(2))
        t0 = time.perf_counter()
        tower = ClipVisionEncoder(layers=args.layers, device=dev)
        tower.load_synthetic(seed=1)
        tower.compile(jit_compile=True)
        plus = IPAdapter.synthetic_plus(5, depth=args.depth, device=dev)
        plus.resampler.compile(jit_compile=True)
        sd = StableDiffusion(args.size, args.size, jit_compile=True, device=dev)
        sd.diffusion_model.load_synthetic(seed=0)
        sd.unconditional_context = unc
        sd.clip_vision = tower
        kw = dict(num_steps=args.steps, unconditional_guidance_scale=7.5, seed=0, guidance_rescale=0.7, return_latent=True, batch_size=1)

        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        picture = rng.integers(0, 256, (480, 640, 3)).astype(np.uint8)
        tok_u, tok_c = sd.image_prompt_tokens(picture, plus)
        sd.generate_image(ctx, ip_adapter=dict(tokens=tok_c, negative_tokens=tok_u, model=plus), **kw)   # warm: the engine built, the loop captured
        job = {"size": args.size, "steps": args.steps, "tower_layers": args.layers, "build_s": round(time.perf_counter() - t0, 1),
               "from_tokens_s": [], "from_picture_first_s": [], "from_picture_repeated_s": []}
        for _ in range(args.rounds):
            other = rng.integers(0, 256, (480, 640, 3)).astype(np.uint8)   # a new picture: preprocess + tower + resampler + job
            job["from_tokens_s"].append(round(timed(lambda: sd.generate_image(ctx, ip_adapter=dict(tokens=tok_c, negative_tokens=tok_u, model=plus), **kw)), 5))
            job["from_picture_first_s"].append(round(timed(lambda: sd.generate_image(ctx, ip_adapter=dict(image=other, model=plus), **kw)), 5))
            job["from_picture_repeated_s"].append(round(timed(lambda: sd.generate_image(ctx, ip_adapter=dict(image=other, model=plus), **kw)), 5))
        m = {k: statistics.median(v) for k, v in job.items() if isinstance(v, list)}
        job["first_minus_tokens_ms"] = round((m["from_picture_first_s"] - m["from_tokens_s"]) * 1e3, 2)
        job["repeated_minus_tokens_ms"] = round((m["from_picture_repeated_s"] - m["from_tokens_s"]) * 1e3, 2)
        out["c_job"] = job   # (the repeated call pays vision.preprocess and the digest, not the networks)
    else:
        out["c_job"] = "not measured (--skip-job)"
    print(json.dumps(out), flush=True)
    save()


if __name__ == "__main__":
    main()
