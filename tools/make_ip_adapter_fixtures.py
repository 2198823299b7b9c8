"""Generate tests/golden/ip_adapter_<size>.npz: the fp32 CPU oracle's final latent of two IP-Adapter image-prompt jobs
(``generate_image(..., ip_adapter=...)``), composed after diffusers' IPAdapterAttnProcessor from pieces that exist without the
product's IP-Adapter code:

  1. the image tokens in torch float64: LayerNorm(768)(Linear(1024 -> 4 * 768)(embeds).reshape(4, 768)) from the synthetic adapter's
     state dict (the public file layout; models.IPAdapter.synthetic_state - a weight table, like the synthetic UNet's), for the
     embedding and for the ZERO embedding (the unconditional forward's tokens);
  2. per step: oracle.sd_oracle.unet_forward for the unconditional and the conditional context.  While a forward runs, this tool has
     wrapped the module attribute sd_oracle.cross_attention by a function that, for names ending ".attn2", computes
     to_out(softmax(q k^T) v + s softmax(q k_ip^T) v_ip) from the same weights, k_ip / v_ip = tokens @ to_k_ip^T / to_v_ip^T of that
     block (checkpoint index 2 j + 1 in diffusers' attn_processors order, written out here by hand), s this step's and block's scale;
     every other name goes to the original (the attribute is restored afterwards; nothing under oracle/ is edited);
  3. eps = u + g (c - u), OracleScheduler.step.

    python tools/make_ip_adapter_fixtures.py            (both sizes)
    python tools/make_ip_adapter_fixtures.py 128        (one)

128x128 px: weight_type "linear"; 256x256 px: weight_type "style" (up_blocks.1 only).  Both: end = 0.75, so the last of the 4 steps
runs at scale 0; batch 1, CFG 7.5, no rescale, the seeded synthetic UNet (seed 0, bias_scale 0.05) and the synthetic adapter
(seed ADAPTER_SEED, 4 tokens).  The contexts are default_rng(CONTEXT_SEED) -> the prompt, then the unconditional context, each
(77, 768); the embedding is default_rng(EMBED_SEED).standard_normal(1024); the noise is default_rng(NOISE_SEED) - what
generate_image(..., seed=NOISE_SEED) draws.

A fixture is only written when the PLAIN job (no adapter) lies under 35 dB against it (`plain_psnr`), so the project's 40 dB bar
tells an image-prompt job from a job without it: the tool walks WEIGHTS upwards until that holds and records the weight.
Nothing of minsdtf_amd is used but the weight tables.
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLD = os.path.join(ROOT, "tests", "golden")
GUIDANCE, STEPS = 7.5, 4
WEIGHT_SEED, BIAS_SCALE, NOISE_SEED, CONTEXT_SEED, EMBED_SEED, ADAPTER_SEED, TOKENS = 0, 0.05, 0, 1234, 77, 5, 4
START, END = 0.0, 0.75
WEIGHTS = (1.0, 1.5, 2.0, 3.0, 4.0)
PLAIN_PSNR_MAX = 35.0
SIZES = {128: "linear", 256: "style"}

# diffusers' attn_processors order of the 16 cross-attentions: the down blocks, the UP blocks, the mid block; entry j is
# ip_adapter.<2 j + 1> of the checkpoint
ORDER = ([f"down_blocks.{lv}.attentions.{r}" for lv in range(3) for r in range(2)]
         + [f"up_blocks.{u}.attentions.{r}" for u in (1, 2, 3) for r in range(3)] + ["mid_block.attentions.0"])
ACTIVE = {"linear": set(ORDER), "style": {f"up_blocks.1.attentions.{r}" for r in range(3)}}


def scale_of(weight, weight_type, block, i):
    """weight inside [START, END) by diffusers' control_guidance rule, times the block factor of the weight type."""
    keep = 0.0 if (i / STEPS < START or (i + 1) / STEPS > END) else 1.0
    return weight * keep * (1.0 if block in ACTIVE[weight_type] else 0.0)


class decoupled:
    """While active, sd_oracle.cross_attention adds the image attention to every attn2, with `scale(block)` and `tokens` (1, N, 768)."""

    def __init__(self, O, state, tokens, scale):
        self.O, self.state, self.tokens, self.scale = O, state, tokens, scale

    def __enter__(self):
        import torch

        O, original = self.O, self.O.cross_attention
        self.original = original

        def cross_attention(x, context, W, name, heads=8):
            if not name.endswith(".attn2"):
                return original(x, context, W, name, heads)
            block = name[:-len(".transformer_blocks.0.attn2")]
            j = ORDER.index(block)
            wk = torch.from_numpy(self.state[f"ip_adapter.{2 * j + 1}.to_k_ip.weight"])
            wv = torch.from_numpy(self.state[f"ip_adapter.{2 * j + 1}.to_v_ip.weight"])
            q = O.dense(x, W, name + ".to_q", bias=False)
            B, S, C = q.shape
            d = C // heads

            def attend(k, v):
                qh = q.view(B, S, heads, d).permute(0, 2, 1, 3)
                kh = k.view(B, -1, heads, d).permute(0, 2, 3, 1)
                vh = v.view(B, -1, heads, d).permute(0, 2, 1, 3)
                return torch.matmul(torch.softmax(torch.matmul(qh, kh) * (d ** -0.5), dim=-1), vh).permute(0, 2, 1, 3).reshape(B, S, C)

            a = attend(O.dense(context, W, name + ".to_k", bias=False), O.dense(context, W, name + ".to_v", bias=False))
            s = self.scale(block)
            if s != 0.0:
                tok = self.tokens.expand(B, -1, -1)
                a = a + s * attend(tok @ wk.t(), tok @ wv.t())
            return O.dense(a, W, name + ".to_out.0")

        O.cross_attention = cross_attention
        return self

    def __exit__(self, *exc):
        self.O.cross_attention = self.original
        return False


def image_tokens(state, embeds):
    import torch

    lin, norm = torch.nn.Linear(1024, TOKENS * 768).double(), torch.nn.LayerNorm(768).double()
    with torch.no_grad():
        lin.weight.copy_(torch.from_numpy(state["image_proj.proj.weight"]))
        lin.bias.copy_(torch.from_numpy(state["image_proj.proj.bias"]))
        norm.weight.copy_(torch.from_numpy(state["image_proj.norm.weight"]))
        norm.bias.copy_(torch.from_numpy(state["image_proj.norm.bias"]))
        return norm(lin(torch.from_numpy(np.asarray(embeds, dtype=np.float64))).reshape(TOKENS, 768)).float()[None]


def run(size):
    import torch

    from minsdtf_amd import weights as Wt
    from minsdtf_amd.models import IPAdapter
    from oracle import sd_oracle as O

    torch.set_num_threads(int(os.environ.get("IP_THREADS", min(16, os.cpu_count() or 1))))
    weight_type = SIZES[size]
    Wn = O.named_weights(Wt.table("civitai_model"), Wt.synth_keras_weights("civitai_model", seed=WEIGHT_SEED, bias_scale=BIAS_SCALE))
    state = IPAdapter.synthetic_state(ADAPTER_SEED, TOKENS)
    h = w = size // 8
    noise = np.random.default_rng(NOISE_SEED).standard_normal((1, h, w, 4)).astype(np.float32)
    rng = np.random.default_rng(CONTEXT_SEED)
    ctx = rng.standard_normal((1, 77, 768)).astype(np.float32)
    unc = rng.standard_normal((1, 77, 768)).astype(np.float32)
    embeds = np.random.default_rng(EMBED_SEED).standard_normal(1024)
    tok_c, tok_u = image_tokens(state, embeds), image_tokens(state, np.zeros(1024))
    original = O.cross_attention
    t0 = time.time()

    def loop(weight):
        s = O.OracleScheduler()
        s.set_timesteps(STEPS)
        x = noise
        for i, t in enumerate(s.timesteps):
            lat = np.asarray(x, dtype=np.float32)
            te = O.timestep_embedding(t, 1)
            scale = lambda block, i=i: scale_of(weight, weight_type, block, i)   # noqa: E731
            with decoupled(O, state, tok_u, scale):
                u = np.asarray(O.unet_forward(Wn, lat, te, unc), dtype=np.float64)
            with decoupled(O, state, tok_c, scale):
                c = np.asarray(O.unet_forward(Wn, lat, te, ctx), dtype=np.float64)
            assert O.cross_attention is original
            x = s.step(u + GUIDANCE * (c - u), t, x)
            print(f"  {size}: weight {weight}, step {i} (t = {t}) done at {time.time() - t0:.0f}s", flush=True)
        return np.asarray(x, dtype=np.float32)

    plain = loop(0.0)
    for weight in WEIGHTS:
        latent = loop(weight)
        plain_psnr = float(O.psnr(plain, latent))
        print(f"{size}: weight {weight} ({weight_type}): the plain job against the image-prompt job: {plain_psnr:.1f} dB", flush=True)
        if plain_psnr >= PLAIN_PSNR_MAX:
            continue
        out = os.path.join(GOLD, f"ip_adapter_{size}.npz")
        np.savez_compressed(out, latent=latent, plain_psnr=plain_psnr, weight=weight, weight_type=weight_type, start=START, end=END, size=size,
                            steps=STEPS, tokens=TOKENS, weight_seed=WEIGHT_SEED, bias_scale=BIAS_SCALE, context_seed=CONTEXT_SEED,
                            embed_seed=EMBED_SEED, adapter_seed=ADAPTER_SEED, noise_seed=NOISE_SEED, guidance=GUIDANCE)
        print("wrote", out, os.path.getsize(out), "bytes in", f"{time.time() - t0:.0f}s", flush=True)
        return
    raise SystemExit(f"{size}: no weight of {WEIGHTS} moves the latent under {PLAIN_PSNR_MAX} dB: extend WEIGHTS")


def main(argv):
    for size in ([int(a) for a in argv] or list(SIZES)):
        run(size)


if __name__ == "__main__":
    main(sys.argv[1:])
