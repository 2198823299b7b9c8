#!/usr/bin/env python3
"""Cost of an IP-Adapter image prompt (generate_image(..., ip_adapter=...), minsdtf_amd/ipadapter.py) on one GPU, seeded synthetic
SD1.5 weights and a synthetic adapter of 4 image tokens:

  (a) the launch - msdi_attention_decoupled at the four level shapes of a 512x512 batch-1 job (2 rows: the guidance pair; 77 text
      keys, N image keys) - as its per-launch period inside a replayed hipGraph, measured twice (A/A), at scale 1 and at scale 0
      (no image key staged), next to
        * msd_attention on the text keys alone (what the launch adds over a plain attention of q),
        * the two-launches-plus-add composition: msd_attention on the text keys, msd_attention on the N image keys, msd_add_bf16
          (an unscaled add: a cost model of the composition, not its arithmetic),
        * the fused msd_cross_attention_q (to_q folded in) the plain job runs at head sizes 40 / 80, against the pair that displaces
          it in an image-prompt job: the to_q GEMM + the decoupled launch;
      all taken inside replayed graphs of 200 launches, best of 5 replays;
  (b) 512x512, 25-step, batch-1 jobs timed in alternation in this one process, each a second time on a pipeline of its own (A/A):
      the plain job and the image-prompt job; the ratio and the difference per step.

    python tools/ip_adapter_bench.py --out profiles/ip_adapter_bench.json
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
# (level name, rows, head size, queries, LayerNorm partial slots of the level's producer GEMM: tools/xattn_bench.py)
LEVELS = [("64x64", 2, 40, 4096, 5), ("32x32", 2, 80, 1024, 10), ("16x16", 2, 160, 256, 10), ("8x8", 2, 160, 64, 20)]


def main(argv=None):
    from regions_bench import graph_period_us, launch_floor_us

    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--tokens", type=int, default=4)
    ap.add_argument("--skip-job", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)

    floor, err = launch_floor_us()   # (first: a child process, before this one opens the GPU)
    import torch

    from minsdtf_amd import host, ops, packing
    from minsdtf_amd.models import IPAdapter
    from minsdtf_amd.stable_diffusion import StableDiffusion

    host.fit_torch_threads()
    dev = torch.device("cuda:0")
    out = {"metric": "ip_adapter", "tokens": args.tokens, "a_launch_floor_us": floor if floor is not None else {"error": err}, "a_launch": []}
    T, H, N = 77, 8, args.tokens
    Tp, Np = (T + 7) // 8 * 8, (N + 7) // 8 * 8
    bf = torch.bfloat16
    step0 = torch.zeros(1, dtype=torch.int32, device=dev)
    for name, B, d, S, slots in LEVELS:
        C = H * d
        gen = torch.Generator().manual_seed(S)
        rn = lambda *shape: torch.randn(*shape, generator=gen)   # noqa: E731
        x = (rn(B * S, C) * 1.5 + 0.3).to(bf).to(dev)
        stats = rn(B * S, slots, 2).abs().to(dev)
        q = (rn(B, S, C) * (d ** -0.5 * 1.4426950408889634)).to(bf).to(dev)
        k, vt = rn(B, T, C).to(bf).to(dev), rn(B, C, Tp).to(bf).to(dev)
        k_ip, vt_ip = rn(B, N, C).to(bf).to(dev), rn(B, C, Np).to(bf).to(dev)
        w0, cs, cb = packing.fold_layer_norm((rn(C, C) / math.sqrt(C)).t().contiguous(), None, torch.ones(C).numpy(), torch.zeros(C).numpy(), dev)
        wq = packing.chunk_major(w0)
        o, o2, q2 = (torch.empty(B, S, C, dtype=bf, device=dev) for _ in range(3))
        geo = dict(batch=B, heads=H, head_dim=d, s=S, q_ld=C, k_ld=C, o_ld=C)

        def ip(scale):
            tab = torch.zeros(1, 16, dtype=torch.float32, device=dev)
            tab[0, 3] = scale
            return ops.ip_attention(q=q, k=k, vt=vt, k_ip=k_ip, vt_ip=vt_ip, out=o, scales=tab, step_ptr=step0, t=T, n=N, vt_ld=Tp, kip_ld=C,
                                    vtip_ld=Np, layer=3, num_steps=1, **geo)

        text = ops.attention(q=q, k=k, vt=vt, out=o, t=T, vt_ld=Tp, scale=1.0, q_prescaled=True, **geo)
        # (the image keys of the composition in buffers of the text context's size: N keys of them are attended to)
        image = ops.attention(q=q, k=rn(B, T, C).to(bf).to(dev), vt=rn(B, C, Tp).to(bf).to(dev), out=o2, t=N, vt_ld=Tp, scale=1.0, q_prescaled=True,
                              **geo)
        add = ops.add_bf16(a=o, b=o2, out=o, n=B * S * C)
        to_q = ops.conv_gemm(a0=x, w=wq, out=q2, batch=1, h_in=B * S, w_in=1, c0=C, N=C, bias=cb, ln_in=stats, ln_in_slots=slots, ln_colsum=cs,
                             w_layout=1)
        ip_q = ops.ip_attention(q=q2, k=k, vt=vt, k_ip=k_ip, vt_ip=vt_ip, out=o, scales=torch.ones(1, 16, dtype=torch.float32, device=dev),
                                step_ptr=step0, t=T, n=N, vt_ld=Tp, kip_ld=C, vtip_ld=Np, layer=3, num_steps=1, **geo)
        forms = {"decoupled": [ip(1.0)], "decoupled_again": [ip(1.0)], "decoupled_scale0": [ip(0.0)], "attention_text": [text],
                 "two_launches_plus_add": [text, image, add], "to_q_plus_decoupled": [to_q, ip_q]}
        if d in (40, 80):
            forms["fused_cross_attention_q"] = [ops.cross_attention_q(x=x, ln_in=stats, ln_in_slots=slots, wq=wq, ln_colsum=cs, bias=cb, k=k, vt=vt,
                                                                      out=o, batch=B, heads=H, head_dim=d, s=S, t=T, k_ld=C, vt_ld=Tp, o_ld=C,
                                                                      w_layout=1)]
        row = {"level": name, "rows": B, "head_dim": d, "s": S, "t": T, "n": N, "workgroups": B * H * ((S + 63) // 64)}
        for form, calls in forms.items():   # (an argument error raises at the first, eager run: nothing was launched or captured)
            row[form + "_us"] = round(graph_period_us(lambda st, cs_=calls: [c(st.cuda_stream) for c in cs_]), 3)
        row["aa_ratio"] = round(max(row["decoupled_us"], row["decoupled_again_us"]) / min(row["decoupled_us"], row["decoupled_again_us"]), 4)
        row["decoupled_over_two_launches"] = round(row["decoupled_us"] / row["two_launches_plus_add_us"], 4)
        row["decoupled_minus_text_us"] = round(row["decoupled_us"] - row["attention_text_us"], 3)
        if "fused_cross_attention_q_us" in row:
            row["pair_minus_fused_us"] = round(row["to_q_plus_decoupled_us"] - row["fused_cross_attention_q_us"], 3)
        out["a_launch"].append(row)
        print(json.dumps(row), flush=True)

    if not args.skip_job:
        rng = np.random.default_rng(0)
        ctx = rng.standard_normal((77, 768)).astype(np.float32)
        unc = rng.standard_normal((77, 768)).astype(np.float32)
        adapter = IPAdapter.synthetic(5, N, device=dev)
        spec = dict(embeds=rng.standard_normal(1024), model=adapter, weight=0.8)
        kinds = {"plain": {}, "ip": dict(ip_adapter=spec)}
        pipes = {}
        for name in [k_ + s_ for k_ in kinds for s_ in ("", "_again")]:   # one pipeline per timed job: each keeps its engine resident
            p = StableDiffusion(args.size, args.size, jit_compile=True, device=dev)
            if pipes:
                p._diffusion_model = next(iter(pipes.values())).diffusion_model
            else:
                p.diffusion_model.load_synthetic(seed=0)
            p.unconditional_context = unc
            pipes[name] = p
        kw = dict(num_steps=args.steps, unconditional_guidance_scale=7.5, seed=0, guidance_rescale=0.7, return_latent=True, batch_size=1)

        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        jobs = {name: (lambda p=p, extra=kinds[name.replace("_again", "")]: p.generate_image(ctx, **extra, **kw)) for name, p in pipes.items()}
        for fn in jobs.values():   # warm: engines built, loops captured
            fn()
        times = {k_: [] for k_ in jobs}
        for _ in range(args.rounds):
            for k_, fn in jobs.items():
                times[k_].append(timed(fn))
        med = {k_: statistics.median(v) for k_, v in times.items()}
        out["b_job"] = {"size": args.size, "batch": 1, "steps": args.steps, "rounds": args.rounds,
                        "launches_per_step": {k_: len(next(iter(pipes[k_]._engines.values())).calls) for k_ in kinds}}
        for k_ in jobs:
            out["b_" + k_ + "_s"] = [round(t, 5) for t in times[k_]]
        out["b_ip_over_plain"] = round(med["ip"] / med["plain"], 4)
        out["b_ip_minus_plain_ms_per_step"] = round((med["ip"] - med["plain"]) * 1e3 / args.steps, 4)
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
