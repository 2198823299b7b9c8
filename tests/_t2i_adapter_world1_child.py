"""Child process of tests/test_t2i_adapter_gpu.py: a ONE-rank torch.distributed process group (backend nccl = RCCL, on cuda:0) whose
exchanges really run (minsdtf_amd.dist.FORCE_COLLECTIVES), as tests/_control_units_world1_child.py sets one up.  A job with a
T2I-Adapter and shard_batch = True then takes the sharded route - the contexts and the noise travel per sample in the packed
broadcast, the scale table travels whole, the features are the rank's own - and must give the bits of the unsharded job.
A fresh interpreter: the process group is created before anything else touches the GPU.  Prints one line `OK {...json...}`."""
import json
import os
import socket
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", LOCAL_RANK="0", WORLD_SIZE="1")
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

    import numpy as np
    import torch
    import torch.distributed as dist

    from minsdtf_amd import dist as mdist

    mdist.FORCE_COLLECTIVES = True
    r, w = mdist.init("nccl", force=True)
    assert (r, w) == (0, 1) and mdist.collectives_on()
    dev = torch.device("cuda", 0)

    from minsdtf_amd.models import T2IAdapter
    from minsdtf_amd.stable_diffusion import StableDiffusion

    sd = StableDiffusion(64, 64, jit_compile=True, device=dev)
    sd.shard_batch = True
    sd.diffusion_model.load_synthetic(seed=0, bias_scale=0.05)
    sd.image_decoder.load_synthetic(seed=0, bias_scale=0.05)
    adapter = T2IAdapter.synthetic(5, 3, device=dev)
    rng = np.random.default_rng(11)
    ctx = rng.standard_normal((77, 768)).astype(np.float32)
    sd.unconditional_context = rng.standard_normal((77, 768)).astype(np.float32)
    spec = dict(image=rng.integers(0, 256, (64, 64, 3)).astype(np.uint8), model=adapter, weight=0.9, end=0.75)
    calls = {"broadcast": 0, "all_gather_into_tensor": 0}
    real = {k: getattr(dist, k) for k in calls}

    def counted(name):
        def f(*a, **k):
            calls[name] += 1
            return real[name](*a, **k)
        return f

    for k in calls:
        setattr(dist, k, counted(k))
    info = {}
    for sampler in ("euler_a",):   # (a stochastic sampler: its draws travel per sample next to the contexts)
        kw = dict(batch_size=2, num_steps=3, unconditional_guidance_scale=7.5, seed=5, guidance_rescale=0.7, sampler=sampler, t2i_adapter=spec)
        n0 = dict(calls)
        mdist.FORCE_COLLECTIVES = True
        forced = sd.generate_image(ctx, **kw)
        forced_latent = sd.generate_image(ctx, return_latent=True, **kw)
        assert calls["broadcast"] >= n0["broadcast"] + 2 and calls["all_gather_into_tensor"] >= n0["all_gather_into_tensor"] + 2, calls
        mdist.FORCE_COLLECTIVES = False
        n1 = dict(calls)
        plain = sd.generate_image(ctx, **kw)
        plain_latent = sd.generate_image(ctx, return_latent=True, **kw)
        assert calls == n1, "the un-forced run must not touch the process group"
        assert forced.shape == (2, 64, 64, 3) and forced.dtype == np.uint8 and forced_latent.shape == (2, 8, 8, 4)
        assert np.array_equal(forced, plain) and np.array_equal(forced_latent, plain_latent), "the collectives changed the result"
        assert len(sd._engines) == 1 and next(iter(sd._engines.values())).t2i_units == 1 and adapter.runs == 1
        assert not np.array_equal(plain_latent, sd.generate_image(ctx, return_latent=True, **{**kw, "t2i_adapter": None})), "the adapter changed nothing"
        info[str(sampler)] = "bit-identical"
    for k in calls:
        setattr(dist, k, real[k])
    mdist.FORCE_COLLECTIVES = True
    info["collectives"] = dict(calls)
    dist.barrier()
    dist.destroy_process_group()
    print("OK " + json.dumps(info), flush=True)


if __name__ == "__main__":
    main()
