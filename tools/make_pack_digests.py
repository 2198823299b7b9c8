#!/usr/bin/env python3
"""Digests of the packed weight image and the LoRA merge plan, for tests/test_pack_layout_cpu.py.

Every launch plan holds raw addresses into the packed image ``HipModel.set_weights`` builds, and the LoRA switch rewrites it in
place, so a change to the packing code must leave every byte and every merge job where it was.  This tool packs each of the seven
model kinds on the host (``device = cpu``, no library), from ``weights.synth_keras_weights(kind, SEED, bias_scale=0.05)``, and writes

* ``tests/golden/pack_digests.json.gz``: per packed key its shape, dtype, whether it is stored chunk-major and the sha256 of its
  bytes; for the UNet and the text encoder (packed with ``lora_switch = True``) the same for every master, every ``ffproj`` top
  block and every saved vector; and the UNet again with ``MFMA_TEMB_PROJ`` off and with ``W_CHUNK_MAJOR`` off;
* ``tests/golden/lora_merge_plan.json.gz``: the merge plan of the UNet and the text encoder (ordered targets and parts, the
  ``ffproj.b`` map, the targetable layers).

Both are gzip-compressed JSON (thousands of digests are data to compare, not text to read; ``zcat`` shows them) and record
the commit they were made from.  To regenerate them from another checkout of this project:

    python tools/make_pack_digests.py --tree /path/to/checkout --write

Without ``--write`` the tool recomputes everything for ``--tree`` (default: this checkout) and reports the keys that differ from
the committed fixtures.
"""
import argparse
import gzip
import hashlib
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SEED = 3
KINDS = ("civitai_model", "controlnet", "hintnet", "decoder", "encoder", "text_clip_embedding", "text_encoder")
SWITCHED = ("civitai_model", "text_encoder")          # packed with lora_switch = True: masters recorded too
# name of the recorded image -> (kind, W_CHUNK_MAJOR, MFMA_TEMB_PROJ)
VARIANTS = dict({k: (k, True, True) for k in KINDS},
                **{"civitai_model/MFMA_TEMB_PROJ=0": ("civitai_model", True, False),
                   "civitai_model/W_CHUNK_MAJOR=0": ("civitai_model", False, True)})


def table_kw(kind):
    return {"clip_skip": -1} if kind == "text_encoder" else {}


def synth(kind):
    from minsdtf_amd import weights

    return weights.synth_keras_weights(kind, SEED, bias_scale=0.05, **table_kw(kind))


def packed_model(kind, arrays, chunk_major=True, mfma_temb_proj=True, lora_switch=False):
    """A model of `kind` with `arrays` set, built without the library: every attribute set_weights needs, on the cpu."""
    from minsdtf_amd import engine, models, weights

    cls = {c.kind: c for c in vars(models).values() if isinstance(c, type) and issubclass(c, models.HipModel) and c.kind}[kind]
    m = cls.__new__(cls)
    m.name, m.device, m._specs = kind, torch.device("cpu"), weights.table(kind, **table_kw(kind))
    m.lora_switch, m._lora, m._W, m._plans, m.weights_version = lora_switch, None, None, {}, 0
    if kind == "text_encoder":
        m.clip_skip = -1
    saved = engine.W_CHUNK_MAJOR, engine.MFMA_TEMB_PROJ
    engine.W_CHUNK_MAJOR, engine.MFMA_TEMB_PROJ = chunk_major, mfma_temb_proj
    try:
        m.set_weights(arrays)
    finally:
        engine.W_CHUNK_MAJOR, engine.MFMA_TEMB_PROJ = saved
    return m


def digest(t, chunk_major=False):
    t = t.detach().contiguous()
    raw = t.view(torch.uint8).numpy().tobytes()
    return [list(t.shape), str(t.dtype).replace("torch.", ""), bool(chunk_major), hashlib.sha256(raw).hexdigest()]


def image_digests(m):
    return {k: digest(t, k in m._W.chunk_major_keys) for k, t in m._W.items()}


def master_digests(m):
    """The LoRA merge's fp32 masters.  The ffproj top blocks are named by their attention block: a tree that keys them by the
    block's ff.net.2 layer records the same names."""
    base = m._lora
    top = {k.replace(".transformer_blocks.0.ff.net.2", ""): t for k, t in base.top.items()}
    return {group: {k: digest(t) for k, t in d.items()} for group, d in (("master", base.master), ("top", top), ("vec", base.vec))}


def merge_plan(plan):
    """A model's LoRA merge plan (model._lora.plan) as plain data, in the order the merge jobs are emitted."""
    flt = lambda q: None if q is None else float(q)  # noqa: E731
    targets = [{"key": t.key, "colsum": t.colsum, "lnb": None if t.lnb is None else list(t.lnb),
                "parts": [{"layer": p.layer, "row_off": int(p.row_off), "col_off": int(p.col_off), "qscale": flt(p.qscale),
                           "colscale": p.colscale, "rowmap": bool(p.rowmap), "ffproj_top": bool(p.ffproj_top)} for p in t.parts]}
               for t in plan.targets]
    return {"targets": targets, "ffproj_b": {k: list(v) for k, v in plan.ffproj_b.items()},
            "layers": {k: [int(x) for x in v] for k, v in plan.layers.items()}}


def compute(names=None, log=lambda s: None):
    """(images, masters, plans) of the recorded variants `names` (default: all); each kind's weights are generated once."""
    images, masters, plans, arrays = {}, {}, {}, {}
    for name in names or VARIANTS:
        kind, cm, mfma = VARIANTS[name]
        if kind not in arrays:
            arrays = {kind: synth(kind)}   # (one kind's fp32 weights alive at a time: the UNet's are 3.4 GB)
        switched = name in SWITCHED
        log(f"packing {name}")
        m = packed_model(kind, arrays[kind], cm, mfma, lora_switch=switched)
        images[name] = image_digests(m)
        if switched:
            masters[name], plans[name] = master_digests(m), merge_plan(m._lora.plan)
    return images, masters, plans


def fixture_path(name):
    return os.path.join(GOLDEN, name + ".json.gz")


def read_fixture(name):
    with gzip.open(fixture_path(name), "rt") as f:
        return json.load(f)


def write_fixture(name, blob):
    with open(fixture_path(name), "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", mtime=0) as f:   # (same bytes every time)
        f.write((json.dumps(blob, separators=(",", ":"), sort_keys=True) + "\n").encode())
    return fixture_path(name)


def differences(want, got, path=""):
    """Names of the leaves (packed keys) that differ between two recorded dicts."""
    if not (isinstance(want, dict) and isinstance(got, dict)):
        return [] if want == got else [path]
    return [d for k in sorted(set(want) | set(got))
            for d in (differences(want[k], got[k], f"{path}/{k}" if path else k) if k in want and k in got
                      else [f"{path}/{k} ({'missing' if k in want else 'unexpected'})"])]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--tree", default=ROOT, help="checkout whose minsdtf_amd is packed (default: this one)")
    ap.add_argument("--write", action="store_true", help="write the fixtures instead of comparing with them")
    args = ap.parse_args()
    tree = os.path.abspath(args.tree)
    sys.path.insert(0, tree)
    # names of the variants ordered so that the three UNet images share one generation of its weights
    order = sorted(VARIANTS, key=lambda n: VARIANTS[n][0])
    images, masters, plans = compute(order, log=lambda s: print(s, file=sys.stderr, flush=True))
    commit = subprocess.run(["git", "-C", tree, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip()
    digests = {"commit": commit, "seed": SEED, "images": images, "masters": masters}
    plan = {"commit": commit, "plans": plans}
    blobs = {"pack_digests": digests, "lora_merge_plan": plan}
    if args.write:
        for name, blob in blobs.items():
            p = write_fixture(name, blob)
            print(f"wrote {p} ({os.path.getsize(p)} bytes)")
        return 0
    bad = []
    for name, blob in blobs.items():
        want = read_fixture(name)
        bad += differences({k: v for k, v in want.items() if k != "commit"}, {k: v for k, v in blob.items() if k != "commit"})
    print("\n".join(bad) if bad else "packed image and merge plan equal the fixtures")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
