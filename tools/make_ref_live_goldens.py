"""G13: what the reference's own code returned in the comparisons that used to run it live inside the CPU tests - its checkpoint
key tables (as digests), its positional loader on the loader tests' generated files, its tokenizer / prompt weighting on seeded random prompts,
and the checkpoints its network code was run on for the G11 fixture.  The tests compare the package against these records, so
they need nothing outside the repository.  The reference is read where it lies (its directory is the one argument) and never
copied; the fixture holds inputs, digests and output arrays only.

    python tools/make_ref_live_goldens.py REFERENCE_DIR    # writes tests/golden/g13_ref_live.json and g13_ref_live_text.npz
"""
import hashlib
import importlib.util
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
OUT_JSON = os.path.join(ROOT, "tests", "golden", "g13_ref_live.json")
OUT_NPZ = os.path.join(ROOT, "tests", "golden", "g13_ref_live_text.npz")

WORDS = ["photo", "graph", "astronaut", "riding", "horse", "moon", "the", "cat's", "Hat", "42", "café", "!!", "...", "(", ")", "[", "]",
         ":1.3)", "\\(", "&amp;", "beautiful", "masterpiece", ",", "\t", "  "]


def array_digest(a):
    """sha256 of one array's shape and float32 bytes."""
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float32))
    h = hashlib.sha256(str(a.shape).encode())
    h.update(a.tobytes())
    return h.hexdigest()


def table_rows_digest(rows):
    """sha256 over an ordered list of (checkpoint key, permutation or None) rows."""
    h = hashlib.sha256()
    for key, perm in rows:
        h.update(json.dumps([key, list(perm) if perm is not None else None]).encode())
    return h.hexdigest()


def key_mapping_digest(mapping):
    """sha256 over a {key: alternative key} dict, in key order."""
    h = hashlib.sha256()
    for k in sorted(mapping):
        h.update(json.dumps([k, mapping[k]]).encode())
    return h.hexdigest()


def checkpoint_digests(path):
    """{key: array_digest} of every tensor of a safetensors file."""
    from safetensors.numpy import load_file

    return {k: array_digest(v) for k, v in sorted(load_file(path).items())}


def graph_checkpoints(tmpdir):
    """The synthetic checkpoints of the G11 VAE / CLIP networks, written exactly as tools/make_ref_graph_goldens.py writes them
    (same seed, bias scale, kinds and file names).  Returns {file name: path}."""
    import torch
    from safetensors.torch import save_file

    import make_ref_graph_goldens as g
    from minsdtf_amd import weights as wtab

    paths = {}
    for name, kinds, kw in (("vae", ("decoder", "encoder"), {}), ("clip_emb", ("text_clip_embedding",), {}),
                            ("text_encoder-1", ("text_encoder",), {"clip_skip": -1}),
                            ("text_encoder-2", ("text_encoder",), {"clip_skip": -2})):
        path = os.path.join(tmpdir, name + ".safetensors")
        if kw:
            sd = {}
            for kind in kinds:
                for spec, w in wtab.synth_tensors(kind, g.SEED, g.BIAS_SCALE, **kw):
                    sd[spec.key] = torch.from_numpy(np.ascontiguousarray(w))
            save_file(sd, path)
        else:
            wtab.write_synthetic_checkpoint(path, kinds=kinds, seed=g.SEED, bias_scale=g.BIAS_SCALE)
        paths[name] = path
    return paths


def random_prompts():
    """The seeded prompts of the tokenizer / weighting comparison: 200 for encode + parse, 25 (with options) for the weighting."""
    rng = np.random.default_rng(5)
    short = [" ".join(rng.choice(WORDS, size=rng.integers(1, 40))) for _ in range(200)]
    long = []
    for _ in range(25):
        s = " ".join(rng.choice(WORDS, size=rng.integers(1, 120)))
        long.append((s, bool(rng.integers(0, 2))))
    return short, long


def _module(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def main():
    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "stable_diffusion")):
        raise SystemExit("usage: python tools/make_ref_live_goldens.py REFERENCE_DIR  (the directory holding stable_diffusion/)")
    ref = os.path.abspath(sys.argv[1])
    import make_goldens as mg
    from minsdtf_amd import weights as W

    out, npz = {}, {}
    ck = _module("ref_ckpt", os.path.join(ref, "stable_diffusion", "ckpt_loader.py"))

    # 1. the checkpoint key tables the loader builds (CKPT_MAPPING / UNET_KEY_MAPPING): row counts and digests, not the tables
    out["ckpt_mapping"] = {kind: {"count": len(rows), "sha256": table_rows_digest(rows)} for kind, rows in ck.CKPT_MAPPING.items()}
    out["unet_key_mapping"] = {"count": len(ck.UNET_KEY_MAPPING), "sha256": key_mapping_digest(ck.UNET_KEY_MAPPING)}

    # 2. the positional loader on the loader tests' generated files: one digest per array it hands to set_weights
    lt = _module("loaders_test", os.path.join(ROOT, "tests", "test_loaders_cpu.py"))
    g8 = json.load(open(os.path.join(ROOT, "tests", "golden", "g8_loaders.json")))
    out["positional_load"] = {}
    for kind, nrows, use_alt, with_lora in lt.CASES:
        with tempfile.TemporaryDirectory() as tmp:
            specs, path, lora = lt._synthetic_case(kind, nrows, use_alt, with_lora, set(g8["lora_unet_keys"]), tmp)
            theirs = mg.FakeKerasModel(kind, specs)
            mapping = ck.CKPT_MAPPING[kind][:nrows] if nrows else ck.CKPT_MAPPING[kind]
            ck.load_weights_from_file(theirs, path, mapping, key_mapping=ck.UNET_KEY_MAPPING if use_alt else None,
                                      lora_dict=dict(lora) if with_lora else None)
        out["positional_load"][f"{kind}-{nrows}-{use_alt}-{with_lora}"] = [array_digest(a) for a in theirs.loaded]

    # 3. the G11 VAE / CLIP fixture: the reference's network code run again over these checkpoints must give the committed arrays
    import make_ref_graph_goldens as g

    g.REF = ref
    base = "/dev/shm" if os.path.isdir("/dev/shm") else None
    with tempfile.TemporaryDirectory(prefix="msd_refgraph_", dir=base) as tmp:
        paths = graph_checkpoints(tmp)
        res, _ = g.reference_outputs(tmp, {"vae", "text"})   # (finds the checkpoints above in tmp; installs the Keras shim)
        out["graph_checkpoints"] = {name: checkpoint_digests(p) for name, p in paths.items()}
    gold = np.load(g.OUT)
    for k, v in res.items():
        e = g.rel_rms(v, gold[k])
        assert e < 1e-6, (k, e)
    out["graph_fixture"] = {k: array_digest(gold[k]) for k in sorted(res)}

    # 4. tokenizer, prompt parsing and weighting on seeded prompts (an inert keras stub replaces the shim: the text modules only import it)
    mg.install_keras_stub()
    sys.path.insert(0, ref)
    import stable_diffusion.clip_tokenizer as ref_tok
    import stable_diffusion.long_prompt_weighting as ref_lpw

    tok = ref_tok.SimpleTokenizer(os.path.join(ROOT, "tests", "golden", "g10_toy_bpe_merges.txt.gz"))
    short, long = random_prompts()
    out["prompts"] = [{"prompt": s, "tokens": tok.encode(s), "parsed": ref_lpw.parse_prompt_attention(s)} for s in short]
    out["weighted"] = []
    for i, (s, no_boseos_middle) in enumerate(long):
        x = ref_lpw.get_weighted_text_embeddings(tok, mg.FakeClipEmbedding(), mg.FakeTextEncoder(), s, no_boseos_middle=no_boseos_middle,
                                                 pad_token_id=tok.end_of_text)
        out["weighted"].append({"prompt": s, "no_boseos_middle": no_boseos_middle, "pad_token_id": tok.end_of_text})
        npz[f"weighted_{i}"] = np.asarray(x)

    with open(OUT_JSON, "w") as f:
        json.dump(out, f, ensure_ascii=False, separators=(",", ":"))
    np.savez_compressed(OUT_NPZ, **npz)
    print("wrote", OUT_JSON, os.path.getsize(OUT_JSON), "bytes;", OUT_NPZ, os.path.getsize(OUT_NPZ), "bytes")


if __name__ == "__main__":
    main()
