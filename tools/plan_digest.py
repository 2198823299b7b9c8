"""Digests of what a DenoiseEngine records, one line per job kind: the check that a change of the plumbing moved no launch.

Run this same file once in a checkout of each commit (it uses only what both have: DenoiseEngine's keyword constructor,
DiffusionModel._build's signature, the engine.Plan.rec hook and the stand-ins of tests/_layer_walk.py) and compare the lines:

    python tools/plan_digest.py          # on the CPU: "<kind>  <recorded launches>  <sha256 over the records>"
    python tools/plan_digest.py --unfolded   # the same with engine.LN_FOLD = engine.FF_PROJ_FOLD = False: the layer_norm routes and
                                             # the unfused attn2 route (the stand-in weights otherwise make every fold "exist")
    python tools/plan_digest.py --run    # on the GPU: "<kind>  <seconds>  <sha256 of the result latent>"

The CPU table has the job kinds first, then "model <kind>": the host loop's twin, DiffusionModel._build at batch 2 and 77 tokens.

A record holds the index of its plan (in the order the plans record their first launch), the op's name, every scalar keyword,
for Buf / BufView / Act operands the arena offset and the bytes available from there, and for operands that are engine tensors
or addresses inside them the engine attribute's name and the byte offset into it.  Default mode: batch 2, 8x8 latent (16x16 for
HyperTile), 3 steps, nothing is launched.  --run: the same kinds through StableDiffusion.generate_image(return_latent=True) on
64x64 pictures (128x128 for HyperTile) with load_synthetic(seed=0) weights and fixed seeds, plus the two kinds that need a side
stream; it stops at the first kind that fails, so run it as one process under one time limit sized from the first kind's time.
"""
import argparse
import hashlib
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np   # noqa: E402
import torch         # noqa: E402

MID = "mid_block.attentions.0"
ADAIN_MID = "mid_block.resnets.1"


# ------------------------------------------------------------------------------------------------------------ the records (CPU)
def _encode(v):
    """One keyword value of a recorded launch -> something whose repr is stable across processes."""
    import _layer_walk as LW
    from minsdtf_amd import engine

    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    if isinstance(v, engine.Act):
        v = v.buf
    if isinstance(v, engine.Buf):
        return ("buf", v.offset, v.nbytes)
    if isinstance(v, engine.BufView):
        return ("buf", v.buf.offset + v.off, v.buf.nbytes - v.off)
    if isinstance(v, engine._Lazy):
        return ("lazy",)
    if isinstance(v, LW._Tensor):
        return ("weight",)
    if isinstance(v, torch.Tensor):
        return ("ptr", v.data_ptr(), ("tensor", tuple(v.shape), str(v.dtype)))
    if type(v).__name__ == "_Ptr":
        return ("ptr", int(v.ptr), ("address",))
    if isinstance(v, np.ndarray):
        return ("array", hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest())
    if isinstance(v, (set, frozenset)):
        return tuple(sorted(_encode(x) for x in v))
    if isinstance(v, (tuple, list)):
        return tuple(_encode(x) for x in v)
    if isinstance(v, dict):
        return tuple((k, _encode(x)) for k, x in sorted(v.items()))
    if isinstance(v, (np.integer, np.floating)):
        return v.item()
    return (type(v).__name__,)


def _engine_tensors(eng):
    """(first byte, bytes, name) of every tensor an engine attribute holds, names sorted."""
    out = []

    def add(name, v):
        if isinstance(v, torch.Tensor):
            if v.numel():
                out.append((v.data_ptr(), v.numel() * v.element_size(), name))
        elif isinstance(v, dict):
            for k in sorted(v, key=str):
                add(f"{name}.{k}", v[k])
        elif isinstance(v, (tuple, list)):
            for i, x in enumerate(v):
                add(f"{name}[{i}]", x)

    for name in sorted(vars(eng)):
        add(name, vars(eng)[name])
    return out


def _resolve(v, tensors):
    """("ptr", address, fallback) -> (attribute name, byte offset) of the engine tensor that holds the address."""
    if isinstance(v, tuple):
        if len(v) == 3 and v[0] == "ptr":
            for p0, nbytes, name in tensors:
                if p0 <= v[1] < p0 + nbytes:
                    return (name, v[1] - p0)
            return v[2]
        return tuple(_resolve(x, tensors) for x in v)
    return v


def record(build):
    """build() -> a DenoiseEngine; returns (number of recorded launches, sha256 over the records)."""
    from minsdtf_amd import engine

    recs, plans = [], {}
    orig = engine.Plan.rec

    def rec(self, fn, **kw):
        recs.append((plans.setdefault(id(self), len(plans)), fn.__name__, tuple((k, _encode(kw[k])) for k in sorted(kw))))
        return orig(self, fn, **kw)

    engine.Plan.rec = rec
    try:
        eng = build()
    finally:
        engine.Plan.rec = orig
    tensors = _engine_tensors(eng)
    h = hashlib.sha256()
    for r in recs:
        h.update(repr(_resolve(r, tensors)).encode())
        h.update(b"\n")
    return len(recs), h.hexdigest()


def stand_ins(h=8, w=8):
    """(UNet, ControlNet, HintNet) stand-ins a DenoiseEngine is fully built from on the CPU."""
    import _layer_walk as LW

    class Tensor(LW._Tensor):
        dtype = torch.bfloat16   # (emit_time_embedding reads it)

    class Weights(LW._AnyWeights):
        def __missing__(self, k):
            return Tensor()

    def net(**kw):
        return types.SimpleNamespace(_require_weights=lambda: None, device=torch.device("cpu"), _W=Weights(), **kw)

    return net(h=h, w=w), net(), net()


def cpu_kinds():
    """(kind, function that builds its engine), in the order of the table."""
    from minsdtf_amd import tiled
    from minsdtf_amd.stable_diffusion import DenoiseEngine

    geo = tiled.parse(dict(size=(64, 128), stride=32), 64, 64)

    def eng(B=2, tc=77, tu=77, g=7.5, phi=0.7, size=8, control=False, **kw):
        unet, cn, hn = stand_ins(size, size)
        if control:
            kw.update(control_net=cn, hint_net=hn)
        return lambda: DenoiseEngine(unet, B, tc, tu, 3, g, phi, **kw)

    return [("plain", eng()), ("guidance 0", eng(g=0.0, phi=0.0)), ("negative prompt of 154 tokens", eng(tu=154)),
            ("euler_a", eng(sampler="euler_a")), ("tcd", eng(tcd=True)), ("inpaint", eng(inpaint=True)),
            ("regions 2 latent", eng(regions=2)), ("regions 3 attention", eng(regions=3, region_mode="attention")),
            ("pag mid", eng(pag=(MID,))), ("reference mid", eng(reference=(MID,))), ("adain alone", eng(adain=(ADAIN_MID,))),
            ("hypertile 2x2", eng(size=16, hypertile=(2, 2, 0))), ("sag", eng(sag=True)), ("sag guidance 0", eng(g=0.0, phi=0.0, sag=True)),
            ("dynthresh", eng(dynthresh=True)), ("dynthresh pag", eng(dynthresh=True, pag=(MID,))),
            ("dynthresh sag", eng(dynthresh=True, sag=True)), ("tiled", eng(B=2 * geo.views, tiled=geo)),
            ("controlnet two passes", eng(tu=154, control=True))]


def model_kinds():
    """(kind, function that builds its bound plan through DiffusionModel._build), in the order of the table."""
    from minsdtf_amd.models import DiffusionModel

    def model(size=8, **kw):
        def build():
            m = DiffusionModel.__new__(DiffusionModel)
            m.h = m.w = size
            m.device, m._W, m._use_graph = torch.device("cpu"), stand_ins()[0]._W, False
            return m._build(2, 77, kw.pop("with_controls", False), **kw)
        return build

    return [("model plain", model()), ("model with_controls", model(with_controls=True)), ("model pag mid", model(pag_layers={MID})),
            ("model regions 2", model(regions=2)), ("model reference mid", model(reference=(MID,))),
            ("model adain alone", model(reference=(), adain=(ADAIN_MID,))), ("model hypertile 2x2", model(size=16, window=(2, 2, 0))),
            ("model sag", model(sag=True))]


# ------------------------------------------------------------------------------------------------------------ the latents (GPU)
def gpu_kinds(dev):
    """(kind, function that runs its job and returns the latent), in the order of the table."""
    from minsdtf_amd import stable_diffusion as sdm
    from minsdtf_amd.models import ControlNet, DiffusionModel, HintNet, ImageEncoder

    nets = {}

    def net(name, cls, *a):
        if name not in nets:
            nets[name] = cls(*a, device=dev)
            nets[name].load_synthetic(seed=0)
        return nets[name]

    rng = np.random.default_rng(11)
    P, Q, S, unc = (rng.standard_normal((77, 768)).astype(np.float32) for _ in range(4))
    neg_long = rng.standard_normal((154, 768)).astype(np.float32)
    picture = rng.integers(0, 256, (64, 64, 3)).astype(np.uint8)
    mask = np.zeros((64, 64), dtype=np.uint8)
    mask[16:48, 8:40] = 255
    y, x = np.mgrid[0:8, 0:8] / 7.0
    two = [dict(prompt=Q, mask=1.0 - x), dict(prompt=S, mask=x + 0.1 * y, weight=2.0)]
    ref_z = rng.standard_normal((1, 8, 8, 4)).astype(np.float32)

    def job(size=64, tcd=False, streams=None, control=False, **kw):
        def run():
            sd = sdm.StableDiffusion(size, size, jit_compile=True, device=dev, active_tcd=tcd,
                                     controlnet_path="synthetic" if control else None)
            sd._diffusion_model = net(f"unet{size}", DiffusionModel, size, size)
            sd._image_encoder = net("enc", ImageEncoder)
            if control:
                sd._control_net, sd._hint_net = net("cn", ControlNet, size, size), net("hn", HintNet, size, size)
                kw["control_net_image"] = picture.astype(np.float32)
            sd.unconditional_context, sd.denoise_streams = unc, streams
            np.random.seed(1234)   # (TCD and un-seeded draws use numpy's global stream)
            args = dict(batch_size=2, num_steps=3, unconditional_guidance_scale=7.5, guidance_rescale=0.7, seed=5, return_latent=True)
            return sd.generate_image(P, **{**args, **kw})
        return run

    dt = dict(mimic_scale=4.0, percentile=0.97)
    return [("plain", job()), ("guidance 0", job(unconditional_guidance_scale=0.0, guidance_rescale=0.0)),
            ("negative prompt of 154 tokens", job(negative_prompt=neg_long)), ("euler_a", job(sampler="euler_a")), ("tcd", job(tcd=True)),
            ("inpaint", job(reference_image=picture, reference_image_strength=0.6, inpaint_mask=mask, mask_blur_strength=3)),
            ("regions 2 latent", job(regions=dict(regions=two))),
            ("regions 3 attention", job(regions=dict(regions=two, base_weight=0.3, mode="attention"))),
            ("pag mid", job(pag=dict(scale=3.0, layers="mid"))), ("reference mid", job(reference_only=dict(latent=ref_z, layers="mid"))),
            ("adain alone", job(reference_only=dict(latent=ref_z, layers=[], adain="auto"))),
            ("hypertile 2x2", job(size=128, hypertile=dict(tile=64, depth=0))), ("sag", job(sag=dict(scale=0.75))),
            ("sag guidance 0", job(sag=dict(scale=0.75), unconditional_guidance_scale=0.0, guidance_rescale=0.0)),
            ("dynthresh", job(dynamic_threshold=dt)), ("dynthresh pag", job(dynamic_threshold=dt, pag=dict(scale=3.0, layers="mid"))),
            ("dynthresh sag", job(dynamic_threshold=dt, sag=dict(scale=0.75))), ("tiled", job(tiled=dict(size=(64, 128), stride=32))),
            ("controlnet two passes", job(control=True, negative_prompt=neg_long)), ("controlnet one fused pass", job(control=True)),
            ("denoise_streams 2", job(streams=2))]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--run", action="store_true", help="run the jobs on the GPU and hash the result latents")
    ap.add_argument("--unfolded", action="store_true", help="record with engine.LN_FOLD = engine.FF_PROJ_FOLD = False")
    ap.add_argument("--save", help="--run: also keep the latents in this .npz (to compare two runs by their largest difference)")
    args = ap.parse_args()
    if not args.run:
        if args.unfolded:
            from minsdtf_amd import engine

            engine.LN_FOLD = engine.FF_PROJ_FOLD = False
        for kind, build in cpu_kinds() + model_kinds():
            n, sha = record(build)
            print(f"{kind:32s} {n:6d}  {sha}", flush=True)
        return
    latents = {}
    for kind, run in gpu_kinds(torch.device("cuda", 0)):
        t0 = time.perf_counter()
        z = np.ascontiguousarray(run(), dtype=np.float32)   # (an exception ends the process here: nothing runs behind a failed kind)
        if not np.isfinite(z).all():
            raise SystemExit(f"{kind}: the latent is not finite")
        latents[kind] = z
        print(f"{kind:32s} {time.perf_counter() - t0:6.1f} s  {hashlib.sha256(z.tobytes()).hexdigest()}", flush=True)
    if args.save:
        os.makedirs(os.path.dirname(os.path.abspath(args.save)), exist_ok=True)
        np.savez(args.save, **latents)


if __name__ == "__main__":
    main()
