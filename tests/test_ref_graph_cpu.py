"""The oracle against the REFERENCE'S OWN network code (G11).

tests/golden/g11_ref_graph.npz holds the outputs of minSDTF's own classes - DiffusionModel (with and without the 13 ControlNet
inputs), ControlNet, HintNet, ImageDecoder, ImageEncoder, TextClipEmbedding, TextEncoder (clip_skip -1 / -2): reference
diffusion_model.py:22-283, layers.py:17-80, image_decoder.py:22-55, image_encoder.py:21-48, control_net.py:10-107,
text_encoder.py:22-169 - executed in the build container over tools/keras_shim.py (an eager torch stand-in for the Keras
primitives: Keras itself is not installable there) on seeded synthetic checkpoints that went through the reference's own
loader and key tables (tools/make_ref_graph_goldens.py).  oracle/sd_oracle.py restates those files by hand; here it must
reproduce the reference code's outputs to fp32 round-off.  Pinned by this: topology, weight placement, every constant the
graph code carries (attention scale, GEGLU constants, quick-GELU 1.702, 1/0.18215, eps, the skip-stack order, the ControlNet
adds).  Not pinned (restated from the Keras documentation on both sides, independently): the inside of Conv2D /
GroupNormalization / LayerNormalization / Dense / UpSampling2D / softmax.
"""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "g11_ref_graph.npz")
TOL = 2e-5   # relative RMS; measured 3e-7 .. 4.1e-6 (fp32 sums in another order)


def _gen():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_ref_graph_goldens as g

    return g


@pytest.mark.timeout(600)
@pytest.mark.parametrize("group", ["vae", "text", "controlnet", "unet"])
def test_oracle_reproduces_the_reference_graph(group):
    g = _gen()
    gold = np.load(GOLD)
    assert (int(gold["seed"]), float(gold["bias_scale"]), int(gold["img"]), int(gold["batch"])) == (g.SEED, g.BIAS_SCALE, g.IMG, g.B)
    got = g.oracle_outputs({group})
    assert got, group
    for k, v in got.items():
        assert v.shape == gold[k].shape and np.isfinite(v).all(), k
        e = g.rel_rms(v, gold[k])
        print(f"{k}: oracle vs reference graph code, relative RMS error {e:.2e}")
        assert e < TOL, (k, e)


def test_the_comparison_has_teeth():
    """The fixture separates what it should: the UNet with ControlNet residuals differs from the one without by far more than
    the tolerance, clip_skip -1 from -2, and the 13 ControlNet outputs are not one tensor repeated."""
    g = _gen()
    gold = np.load(GOLD)
    assert g.rel_rms(gold["unet_controls"], gold["unet"]) > 100 * TOL
    assert g.rel_rms(gold["text_encoder-2"], gold["text_encoder-1"]) > 100 * TOL
    assert g.rel_rms(gold["controlnet.1"], gold["controlnet.0"]) > 100 * TOL
    assert float(np.abs(gold["decoder"]).max()) > 1e-3 and float(np.abs(gold["encoder"]).max()) > 1e-3


@pytest.mark.timeout(900)
def test_live_reference_graph_matches_the_fixture(tmp_path):
    """The fixture's VAE / CLIP arrays are what the reference's code computed, over the shim, from the checkpoints this repository
    writes today: tools/make_ref_live_goldens.py ran the reference's networks again on checkpoints it wrote itself, checked the
    outputs against the committed fixture, and recorded a digest of every tensor of those checkpoints and of every fixture array it
    checked (tests/golden/g13_ref_live.json).  Here the checkpoints are written again and must carry the recorded tensors, and the
    fixture must still hold the recorded arrays (the name is from when the reference ran here; the UNet's turn needs its 3.4 GB
    synthetic checkpoint and stays with `python tools/make_ref_graph_goldens.py --check`)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_ref_live_goldens as rl

    rec = json.load(open(os.path.join(ROOT, "tests", "golden", "g13_ref_live.json")))
    paths = rl.graph_checkpoints(str(tmp_path))
    assert sorted(paths) == sorted(rec["graph_checkpoints"])
    for name, path in paths.items():
        got, want = rl.checkpoint_digests(path), rec["graph_checkpoints"][name]
        assert sorted(got) == sorted(want), name
        bad = [k for k in want if got[k] != want[k]]
        assert not bad, (name, bad[:5])
        os.remove(path)
    gold = np.load(GOLD)
    assert set(rec["graph_fixture"]) == {"decoder", "encoder", "clip_embedding", "text_encoder-1", "text_encoder-2"}
    for k, d in rec["graph_fixture"].items():
        assert rl.array_digest(gold[k]) == d, k
