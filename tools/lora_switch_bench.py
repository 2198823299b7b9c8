"""Cost of a LoRA switch (StableDiffusion.set_loras, minsdtf_amd/lora.py) against today's route, at 512x512 from a synthetic checkpoint
file, with two synthetic rank-32 LoRAs over all 278 UNet layers and the 72 text-encoder layers:

  (a) set_loras, alternating the two LoRAs: median wall time of the call, and the msd_lora_merge kernel's own GPU time with its
      fraction of an HBM floor (bytes = masters read + packed and fragment-major images written + factors read);
  (b) today's route: a new StableDiffusion(lora_path=) through its first finished 25-step job;
  (c) 25-step images/s of the captured loop before and after a switch.

    python tools/lora_switch_bench.py --out profiles/lora_switch_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12   # MI355X HBM3E peak, bytes / s


def lora_state_dict(seed, rank=32, std=0.02):
    from minsdtf_amd import weights as Wt

    rng = np.random.default_rng(seed)
    spec_of = {s.alt_key: s for s in Wt.table("civitai_model") if s.alt_key}
    items = [(n, spec_of[k].torch_shape) for n, k in Wt._lora_unet_name_map().items()]
    items += [("lora_te_" + s.name.replace(".", "_"), s.torch_shape) for s in Wt.table("text_encoder")
              if s.kind == "dense_w" and s.name.endswith(Wt._LORA_TE_SUFFIXES)]
    sd = {}
    for n, ts in items:
        up, down = ((ts[0], rank), (rank, ts[1])) if len(ts) == 2 else ((ts[0], rank, 1, 1), (rank, ts[1], ts[2], ts[3]))
        sd[n + ".lora_up.weight"] = torch.from_numpy((rng.standard_normal(up) * std).astype(np.float32))
        sd[n + ".lora_down.weight"] = torch.from_numpy((rng.standard_normal(down) * std).astype(np.float32))
        sd[n + ".alpha"] = torch.tensor(float(rank))
    return sd


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--switches", type=int, default=10)
    ap.add_argument("--jobs", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)

    from safetensors.torch import save_file

    from minsdtf_amd import host, ops
    from minsdtf_amd import weights as Wt
    from minsdtf_amd.stable_diffusion import StableDiffusion

    host.fit_torch_threads()
    dev = torch.device("cuda:0")
    tmp = tempfile.mkdtemp(prefix="lora_bench_")
    ck = os.path.join(tmp, "sd15.safetensors")
    Wt.write_synthetic_checkpoint(ck, kinds=("civitai_model", "decoder", "text_encoder", "text_clip_embedding"), seed=0,
                                  bias_scale=0.05)
    la, lb = os.path.join(tmp, "a.safetensors"), os.path.join(tmp, "b.safetensors")
    save_file(lora_state_dict(1), la)
    save_file(lora_state_dict(2), lb)
    h = w = args.size // 8
    rng = np.random.default_rng(0)
    ctx = rng.standard_normal((77, 768)).astype(np.float32)
    unc = rng.standard_normal((77, 768)).astype(np.float32)
    noise = rng.standard_normal((h, w, 4)).astype(np.float32)

    def job(sd):
        sd.unconditional_context = unc
        return sd.generate_image(ctx, batch_size=1, num_steps=args.steps, unconditional_guidance_scale=7.5, diffusion_noise=noise,
                                 guidance_rescale=0.7, return_latent=True)

    def ips(sd):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.jobs):
            job(sd)
        torch.cuda.synchronize()
        return args.jobs / (time.perf_counter() - t0)

    # (b) today's route: construction (file read, host packing, upload) + the first job (plans, capture)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    old = StableDiffusion(args.size, args.size, jit_compile=True, unet_ckpt=ck, text_encoder_ckpt=ck, vae_ckpt=ck, lora_path=la,
                          device=dev)
    job(old)
    torch.cuda.synchronize()
    reload_s = time.perf_counter() - t0
    del old
    import gc

    gc.collect()
    torch.cuda.empty_cache()

    sd = StableDiffusion(args.size, args.size, jit_compile=True, unet_ckpt=ck, text_encoder_ckpt=ck, vae_ckpt=ck,
                         lora_switch=True, device=dev)
    sd.text_encoder   # (loaded: its layers switch too)
    job(sd)   # capture
    before = ips(sd)

    # kernel-only time: events around every msd_lora_merge launch, bytes from its job descriptors
    kernel = []
    real = ops.lora_merge

    def timed(jobs, device, name="lora_merge"):
        call = real(jobs, device)
        nbytes = 0
        for j in jobs:
            el = j.n * j.k
            nbytes += el * 4 + el * (4 if j.out_dtype == ops.OUT_F32 else 2) + (el * 2 if j.out_frag else 0)
            nbytes += (j.n + j.k) * j.rank * 4
        fn = call.fn

        def run(*a):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            rc = fn(*a)
            e.record()
            kernel.append((s, e, nbytes, len(jobs)))
            return rc
        call.fn = run
        return call

    ops.lora_merge = timed
    sd.set_loras([(la, 1.0)])
    sd.set_loras([(lb, 1.0)])   # (both files read and cached)
    kernel.clear()
    walls = []
    for i in range(args.switches):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sd.set_loras([(la if i % 2 == 0 else lb, 1.0)])
        walls.append(time.perf_counter() - t0)
    ops.lora_merge = real
    torch.cuda.synchronize()
    ks = [s.elapsed_time(e) * 1e-3 for s, e, _b, _n in kernel]
    # one switch = one launch per model (UNet, text encoder): sum them per switch
    nmod = len(kernel) // args.switches
    sw_k = [sum(ks[i * nmod:(i + 1) * nmod]) for i in range(args.switches)]
    sw_b = [sum(b for _s, _e, b, _n in kernel[i * nmod:(i + 1) * nmod]) for i in range(args.switches)]
    k_med = statistics.median(sw_k)
    after = ips(sd)
    out = {
        "metric": "lora_switch", "size": args.size, "steps": args.steps, "rank": 32, "layers": {"unet": 278, "text_encoder": 72},
        "a_set_loras_wall_ms_median": round(statistics.median(walls) * 1e3, 2),
        "a_set_loras_wall_ms_all": [round(x * 1e3, 2) for x in walls],
        "a_kernel_ms_median": round(k_med * 1e3, 3), "a_launches_per_switch": nmod,
        "a_kernel_bytes": int(sw_b[0]), "a_hbm_floor_ms": round(sw_b[0] / HBM_PEAK * 1e3, 3),
        "a_hbm_fraction": round(sw_b[0] / HBM_PEAK / k_med, 3),
        "b_reload_through_first_job_s": round(reload_s, 2),
        "c_images_per_s_before_switch": round(before, 4), "c_images_per_s_after_switch": round(after, 4),
        "c_after_over_before": round(after / before, 4),
    }
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
