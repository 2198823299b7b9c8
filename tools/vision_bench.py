#!/usr/bin/env python3
"""Cost and accuracy of the CLIP ViT-H/14 vision tower (models.ClipVisionEncoder, minsdtf_amd/vision.py) on one GPU, seeded synthetic
weights.  Every period is taken inside a replayed hipGraph; every series is measured twice in alternation (A/A).

  (a) the launch floor (tools/launch_floor.py, a child process) and each new kernel of libminsdtf_hip_vision.so at the tower's shapes;
  (b) the 32-layer tower at batch 1: its replayed graph, two bound plans of the one model timed in alternation; its floor = launch
      floor x launch count + weight bytes / 8 TB/s; and where the time goes: every launch of one layer at its shape, each in a graph of
      its own (the layer's weights then stay in the caches: a lower bound of its share, said so in the output);
  (c) the final embedding at full depth against vision.forward_host (float64), as PSNR;
  (d) an ip_adapter job from a picture (512x512, 25 steps, batch 1) on its first and its repeated call, next to the job from embeds;
  (e) with --parent DIR (a built checkout of the parent commit): bench.py there and here in alternation, fresh processes.

    python tools/vision_bench.py --out profiles/clip_vision_bench.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
HBM_BYTES_PER_S = 8.0e12


def bench_ab(parent, steps, warmup, rounds):
    """bench.py --gpus 1 in `parent` and here, in alternation, each a fresh process: images/s per run."""
    runs = {"parent": [], "here": []}
    for _ in range(rounds):
        for name, cwd in (("parent", parent), ("here", ROOT)):
            try:
                out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)], cwd=cwd, check=True,
                                     stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900).stdout
                line = [ln for ln in out.splitlines() if ln.startswith("{")][-1]
                runs[name].append(json.loads(line))
            except (OSError, subprocess.SubprocessError, IndexError, ValueError) as e:
                runs[name].append({"error": f"{type(e).__name__}: {e}"[:300]})
    return runs


def main(argv=None):
    from regions_bench import graph_period_us, launch_floor_us

    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip-job", action="store_true")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: bench.py there and here in alternation")
    ap.add_argument("--bench-only", action="store_true", help="with --parent and --out: only (e), merged into the existing --out file")
    ap.add_argument("--bench-steps", type=int, default=10)
    ap.add_argument("--bench-warmup", type=int, default=2)
    ap.add_argument("--bench-rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)

    out = {"metric": "clip_vision", "layers": args.layers}
    if args.bench_only:
        if not (args.parent and args.out):
            ap.error("--bench-only goes with --parent and --out")
        if os.path.exists(args.out):
            out = json.load(open(args.out))
        out["e_bench"] = bench_ab(args.parent, args.bench_steps, args.bench_warmup, args.bench_rounds)
        ips = {k: [r.get("value") for r in v] for k, v in out["e_bench"].items()}
        out["e_bench_images_per_s"] = ips
        print(json.dumps(ips), flush=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
        return
    if args.parent:   # (first: child processes, before this one opens the GPU)
        out["e_bench"] = bench_ab(args.parent, args.bench_steps, args.bench_warmup, args.bench_rounds)
        print(json.dumps(out["e_bench"]), flush=True)
    else:
        out["e_bench"] = "not measured (no --parent checkout given)"
    floor, err = launch_floor_us()
    import torch

    from minsdtf_amd import host, vision
    from minsdtf_amd.models import ClipVisionEncoder, IPAdapter
    from minsdtf_amd.stable_diffusion import StableDiffusion

    host.fit_torch_threads()
    dev = torch.device("cuda:0")
    out["a_launch_floor_us"] = floor if floor is not None else {"error": err}
    rng = np.random.default_rng(0)
    picture = rng.integers(0, 256, (480, 640, 3)).astype(np.uint8)
    px = vision.preprocess(picture)

    # ---- (b) the tower
    t0 = time.perf_counter()
    tower = ClipVisionEncoder(layers=args.layers, device=dev)
    state = tower.load_synthetic(seed=1)
    tower.compile(jit_compile=True)
    out["b_build_s"] = round(time.perf_counter() - t0, 2)
    emb = tower.predict_on_batch(px[None])                                   # plan A, captured
    hid = tower.predict_on_batch(px[None], output="last_hidden_state")       # plan B: the same launches, a cast for the pooled head
    plans = {"tower": tower._bound((1, "image_embeds"), None), "tower_again": tower._bound((1, "last_hidden_state"), None)}
    times = {k: [] for k in plans}
    for _ in range(args.rounds):
        for k, bp in plans.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            bp.graph.replay()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3)
    launches = len(plans["tower"].plan.calls)
    wbytes = sum(int(t.numel()) * t.element_size() for t in tower._W.values() if isinstance(t, torch.Tensor))
    med = {k: statistics.median(v) for k, v in times.items()}
    both = times["tower"] + times["tower_again"]
    out["b_tower"] = {"batch": 1, "launches": launches, "weight_bytes": wbytes, "rounds": args.rounds,
                      "tower_us": [round(t, 1) for t in times["tower"]], "tower_again_us": [round(t, 1) for t in times["tower_again"]],
                      "median_us": round(med["tower"], 1), "aa_ratio": round(med["tower_again"] / med["tower"], 4),
                      "aa_spread": round((max(both) - min(both)) / statistics.median(both), 4),
                      "weights_at_8TBs_us": round(wbytes / HBM_BYTES_PER_S * 1e6, 1)}
    if floor is not None:
        fl = floor * launches + wbytes / HBM_BYTES_PER_S * 1e6
        out["b_tower"].update(floor_us=round(fl, 1), over_floor=round(med["tower"] / fl, 3))
    print(json.dumps(out["b_tower"]), flush=True)
    # where the time goes: the launches of layer 0 (calls 1 .. 8 of the plan) and the two ends, each alone in a replayed graph
    calls = plans["tower"].plan.calls
    share = {}
    for i in [0] + list(range(1, 9)) + [launches - 1]:
        c = calls[i]
        name = c.name.replace("vision_model.encoder.layers.0.", "layer.").replace("vision_model.", "")
        a = graph_period_us(lambda st, c_=c: c_(st.cuda_stream), n=50)
        b = graph_period_us(lambda st, c_=c: c_(st.cuda_stream), n=50)
        share[name] = {"us": round(a, 2), "again_us": round(b, 2)}
    per_layer = sum(v["us"] for k, v in share.items() if k.startswith("layer."))
    out["b_launches_hot_weights"] = share
    out["b_layer_sum_hot_us"] = round(per_layer, 1)
    out["b_note"] = ("a launch repeated in its own graph re-reads the same weights from the caches: layer_sum_hot x layers is a lower bound of "
                     "the tower; the rest of the measured period is weight streaming from HBM and the M = 257 tail of the GEMM tiles")
    print(json.dumps(share), flush=True)

    # ---- (a) the new kernels at the tower's shapes (patch_embed B = 1, gelu 257 x 5120, pool_project B = 1) are calls 0, 7, last
    out["a_kernels"] = {k: share[n] for k, n in (("patch_embed", "embeddings"), ("gelu", "layer.mlp.gelu"), ("pool_project", "visual_projection"))}
    if floor is not None:
        for v in out["a_kernels"].values():
            v["over_launch_floor"] = round(v["us"] / floor, 2)

    # ---- (c) accuracy at full depth
    t0 = time.perf_counter()
    ref = vision.forward_host(state, px[None], args.layers)
    from oracle import sd_oracle as O

    out["c_psnr_db"] = {"image_embeds": round(O.psnr(emb, ref["image_embeds"]), 2), "last_hidden_state": round(O.psnr(hid, ref["last_hidden_state"]), 2),
                        "forward_host_s": round(time.perf_counter() - t0, 1)}
    print(json.dumps(out["c_psnr_db"]), flush=True)

    # ---- (d) the job from a picture
    if not args.skip_job:
        ctx = rng.standard_normal((77, 768)).astype(np.float32)
        unc = rng.standard_normal((77, 768)).astype(np.float32)
        adapter = IPAdapter.synthetic(5, 4, device=dev)
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

        e = sd.encode_image_prompt(picture)
        sd.generate_image(ctx, ip_adapter=dict(embeds=e, model=adapter), **kw)   # warm: the engine built, the loop captured
        job = {"size": args.size, "steps": args.steps, "from_embeds_s": [], "from_picture_first_s": [], "from_picture_repeated_s": []}
        for i in range(args.rounds):
            other = rng.integers(0, 256, (480, 640, 3)).astype(np.uint8)   # a new picture: preprocess + tower + job
            job["from_embeds_s"].append(round(timed(lambda: sd.generate_image(ctx, ip_adapter=dict(embeds=e, model=adapter), **kw)), 5))
            job["from_picture_first_s"].append(round(timed(lambda: sd.generate_image(ctx, ip_adapter=dict(image=other, model=adapter), **kw)), 5))
            job["from_picture_repeated_s"].append(round(timed(lambda: sd.generate_image(ctx, ip_adapter=dict(image=other, model=adapter), **kw)), 5))
        m = {k: statistics.median(v) for k, v in job.items() if isinstance(v, list)}
        job["first_minus_embeds_ms"] = round((m["from_picture_first_s"] - m["from_embeds_s"]) * 1e3, 2)
        job["repeated_minus_embeds_ms"] = round((m["from_picture_repeated_s"] - m["from_embeds_s"]) * 1e3, 2)
        out["d_job"] = job
    else:
        out["d_job"] = "not measured (--skip-job)"
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
