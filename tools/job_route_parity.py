"""Bit parity of every generate_image job route between two commits, and the host-side cost of a repeated resident job.

Run this same file once in a checkout of each commit (it uses only what both have: the public API, `_engines`, `.calls`):

    python tools/job_route_parity.py --out head.json [--time 20]

64x64 pipeline, synthetic weights (seed 0, bias_scale 0.05), fixed contexts, 3-4 steps.  Per job: the SHA-256 of the
`return_latent=True` result and of the uint8 image, and for every engine resident afterwards the digest of its launch names and
their number.  `--time N`: the wall clock of N repeats of the resident plain / hires / tiled / regional job (return_latent=True, each
ends in its device-to-host copy), three rounds each.  Two outputs are equal when their "jobs" sections are equal entry for entry.
"""
import argparse
import hashlib
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np   # noqa: E402
import torch         # noqa: E402


def digest(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--time", type=int, default=0, help="repeats per timed round of the resident jobs (0: none)")
    args = ap.parse_args()
    from minsdtf_amd import stable_diffusion as sdm
    from minsdtf_amd.models import ControlNet, DiffusionModel, HintNet, ImageDecoder, ImageEncoder

    dev = torch.device("cuda", 0)
    nets = {}
    for name, cls, a in (("unet", DiffusionModel, (64, 64)), ("dec", ImageDecoder, ()), ("enc", ImageEncoder, ()),
                         ("cn", ControlNet, (64, 64)), ("hn", HintNet, (64, 64))):
        nets[name] = cls(*a, device=dev)
        nets[name].load_synthetic(seed=0, bias_scale=0.05)
    rng = np.random.default_rng(11)
    P, Q, S = (rng.standard_normal((77, 768)).astype(np.float32) for _ in range(3))
    unc = rng.standard_normal((77, 768)).astype(np.float32)
    neg_long = rng.standard_normal((154, 768)).astype(np.float32)
    picture = rng.integers(0, 256, (64, 64, 3)).astype(np.uint8)
    mask = np.zeros((64, 64), dtype=np.uint8)
    mask[16:48, 8:40] = 255
    y, x = np.mgrid[0:8, 0:8] / 7.0
    region_list = [dict(prompt=Q, mask=1.0 - x), dict(prompt=S, mask=x + 0.1 * y, weight=2.0)]
    hires = dict(scale=2, steps=4, strength=0.5, upscaler="bicubic")
    tiled = dict(size=(64, 128), stride=32, blend="gaussian")

    def pipe(jit=True, tcd=False, streams=None, control=False):
        sd = sdm.StableDiffusion(64, 64, jit_compile=jit, device=dev, active_tcd=tcd, controlnet_path="synthetic" if control else None)
        sd._diffusion_model, sd._image_decoder, sd._image_encoder = nets["unet"], nets["dec"], nets["enc"]
        if control:
            sd._control_net, sd._hint_net = nets["cn"], nets["hn"]
        sd.unconditional_context, sd.denoise_streams = unc, streams
        return sd

    base = dict(batch_size=2, num_steps=4, unconditional_guidance_scale=7.5, guidance_rescale=0.7, seed=5)
    jobs = {}

    def record(name, sd, **kw):
        kw = {**base, **kw}
        if "diffusion_noise" in kw:
            kw.pop("seed")
        out = {}
        for what, extra in (("latent", dict(return_latent=True)), ("image", {})):
            np.random.seed(1234)   # (TCD and un-seeded draws use numpy's global stream)
            out[what] = digest(sd.generate_image(P, **kw, **extra))
        out["engines"] = [[hashlib.sha256("\n".join(c.name for c in e.calls).encode()).hexdigest(), len(e.calls)]
                          for e in sd._engines.values()]
        jobs[name] = out
        print(name, out["latent"][:12], out["image"][:12], [n for _d, n in out["engines"]], flush=True)

    sd = pipe()
    record("plain", sd)
    record("guidance 0", sd, unconditional_guidance_scale=0.0)
    record("negative context of another length", sd, negative_prompt=neg_long)
    record("callback", sd, callback=lambda i: None)
    for s in ("dpmpp_2m_karras", "euler_a"):
        record(f"sampler {s}", sd, sampler=s)
    record("euler_a without a seed", sd, sampler="euler_a", diffusion_noise=rng.standard_normal((2, 8, 8, 4)).astype(np.float32))
    record("image to image", sd, reference_image=picture, reference_image_strength=0.6)
    record("image to image euler_a", sd, reference_image=picture, reference_image_strength=0.6, sampler="euler_a")
    record("inpaint", sd, reference_image=picture, reference_image_strength=0.6, inpaint_mask=mask, mask_blur_strength=3)
    for s in (None, "dpmpp_2m_karras", "euler_a"):
        record(f"hires {s}", sd, hires=hires, sampler=s)
    record("tiled euler_a", sd, tiled=tiled, sampler="euler_a")
    record("tiled", sd, tiled=tiled)
    record("regions", sd, regions=dict(regions=region_list))
    record("regions with a base weight", sd, regions=dict(regions=region_list, base_weight=0.3))
    record("regions euler_a", sd, regions=dict(regions=region_list, base_weight=0.3), sampler="euler_a")
    record("host loop", sd, host_loop=True)
    record("host loop dpmpp_2m_karras", sd, host_loop=True, sampler="dpmpp_2m_karras")
    record("host loop regions", sd, host_loop=True, regions=dict(regions=region_list, base_weight=0.3))
    record("plain again", sd)
    record("hires after a plain job", sd, hires=hires)
    record("two streams", pipe(streams=2))
    record("no graph", pipe(jit=False))
    record("tcd", pipe(tcd=True))
    record("tcd image to image", pipe(tcd=True), reference_image=picture, reference_image_strength=0.6)
    for overlap in (True, False):
        sdm.CONTROLNET_OVERLAP = overlap
        record(f"controlnet overlap {int(overlap)}", pipe(control=True), control_net_image=picture.astype(np.float32))
        record(f"controlnet host loop {int(overlap)}", pipe(control=True), control_net_image=picture.astype(np.float32), host_loop=True)
    sdm.CONTROLNET_OVERLAP = True

    result = {"jobs": jobs}
    if args.time:
        timed = {"plain": {}, "hires": dict(hires=hires), "tiled": dict(tiled=tiled),
                 "regions": dict(regions=dict(regions=region_list, base_weight=0.3))}
        result["repeat_seconds"] = {}
        for name, extra in timed.items():
            kw = {**base, **extra, "return_latent": True}
            sd.generate_image(P, **kw)
            sd.generate_image(P, **kw)   # resident: nothing is built or captured from here on
            rounds = []
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.time):
                    sd.generate_image(P, **kw)   # (ends in the result's device-to-host copy)
                rounds.append(time.perf_counter() - t0)
            result["repeat_seconds"][name] = rounds
            print("repeat", name, args.time, "calls:", ["%.4f" % r for r in rounds], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
