"""Measure the two kernel errors of self-attention guidance over the cases of tests/test_sag_gpu.py and write
profiles/sag_parity.json: the maximum relative error of msdx_attention_colsum against the float64 softmax of the same bf16
operands, and the maximum error (relative to max |reference|) of msdx_sag_degrade against sag.degrade_host.  The tests' bounds are
4 x these figures: the kernels are deterministic, the margin covers other seeds.

    python tools/sag_parity.py [--out profiles/sag_parity.json]        (needs the GPU)
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sag_parity.json"))
    args = ap.parse_args()
    import torch

    import test_sag_gpu as T
    from minsdtf_amd import sag

    gpu = torch.device("cuda", 0)
    cs = {}
    for shape in T.COLSUM_SHAPES:
        q, k = T.colsum_inputs(shape)
        got, _g = T.colsum_run(gpu, shape, q, k)
        cs["x".join(str(v) for v in shape)] = T.colsum_error(got, T.colsum_reference(q[1:], k[1:], shape[1]))
        print("colsum", shape, cs["x".join(str(v) for v in shape)], flush=True)
    dg = {}
    for shape in T.DEGRADE_SHAPES:
        for stride in (4, 8):
            for kind in ("all", "mixed"):
                x, e, coef, A = T.degrade_inputs(shape, stride, kind)
                got, par = T.degrade_run(gpu, shape, stride, x, e, coef, A)
                ref = sag.degrade_host(x, e, coef[1, 0], coef[1, 1], A, shape[2:], par[:9], par[9])
                key = "x".join(str(v) for v in shape) + f"/stride{stride}/{kind}"
                dg[key] = T.degrade_error(got, ref)
                print("degrade", key, dg[key], flush=True)
    out = dict(colsum_max_rel_err=max(cs.values()), degrade_max_err=max(dg.values()), colsum=cs, degrade=dg,
               note="maxima over the cases of tests/test_sag_gpu.py; the tests' bounds are 4 x the two maxima")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
